"""ctypes binding of the C ABI in include/kmerhip.h (krust_amd/lib/libkmerhip.so).

This is plumbing only: every call goes to the hand-written HIP path.  There is
no CPU fallback -- if the shared library is missing, or no HIP device is usable,
the calls fail loudly (ImportError / KmerHipError).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", os.environ.get("KMERHIP_LIB", "libkmerhip.so"))  # KMERHIP_LIB: A/B builds

KH_OK = 0
KH_ERR_BAD_K = -1
KH_ERR_BAD_ARG = -2
KH_ERR_NO_DEVICE = -3
KH_ERR_OOM = -4
KH_ERR_TABLE_FULL = -5
KH_ERR_HIP = -6
KH_ERR_STATE = -7
KH_ERR_RANGE = -8
KH_ERR_FORMAT = -9
KH_ERR_RCCL = -10
KH_ERR_PEER = -11
TEXT_FASTA, TEXT_FASTQ = 1, 2
KH_OUT_FASTA, KH_OUT_TSV, KH_OUT_JSON = 1, 2, 3  # kh_result_text_begin
KH_OUT_SORTED = 0x100  # ... ORed into the format: records in ascending key order
PROFILE_NO_WINDOW = 0xFFFFFFFF  # KH_PROFILE_NO_WINDOW: an entry of kh_profile* where counting would see no window
# KH_REC_*: the words of a row of kh_profile_records*
REC_WORDS = 8
REC_WINDOWS, REC_PRESENT, REC_IN_RANGE, REC_MIN, REC_MAX, REC_SUM_LO, REC_SUM_HI, REC_FIRST_LOW = range(8)
# KH_CMP_*: the words of kh_compare; KH_SET_* / KH_CALC_*: the set operations and count rules of kh_combine_into
CMP_WORDS = 8
CMP_DISTINCT_A, CMP_DISTINCT_B, CMP_SHARED, CMP_SUM_A, CMP_SUM_B, CMP_SHARED_SUM_A, CMP_SHARED_SUM_B, CMP_SUM_MIN = range(8)
CMP_NAMES = ("distinct_a", "distinct_b", "shared", "sum_a", "sum_b", "shared_sum_a", "shared_sum_b", "sum_min")
SET_INTERSECT, SET_UNION, SET_SUBTRACT, SET_COUNT_SUBTRACT = 1, 2, 3, 4
CALC_MIN, CALC_MAX, CALC_SUM, CALC_LEFT, CALC_RIGHT = 1, 2, 3, 4, 5
# KH_GRAPH_*: the words of kh_graph_stats -- [m], m < 256: nodes whose mask is m -- and the bits of a mask (kh_graph_masks*)
GRAPH_WORDS, GRAPH_NODES, GRAPH_KMERS = 258, 256, 257


def GRAPH_RIGHT(c):
    """The mask bit of the right neighbour by letter c (0..3 = A, C, G, T)."""
    return 1 << c


def GRAPH_LEFT(c):
    return 16 << c


# KH_UNI_*: the words of a unitig row (kh_unitigs_*)
UNI_WORDS, UNI_START, UNI_KMERS, UNI_COUNT_SUM, UNI_FLAGS = 4, 0, 1, 2, 3
UNI_CIRCULAR = 1
# KH_UNI_TEXT_*: the formats of kh_unitigs_text_begin; UNI_TEXT_TILE: the bytes of the document one workgroup formats (UT_TILE of
# krust_amd/csrc/unitig_text.hip.h) -- the tests place records on its edges
KH_UNI_TEXT_FASTA, KH_UNI_TEXT_GFA = 1, 2
UNI_TEXT_TILE = 8192


# KH_UNI_LINK_*: a link word of kh_unitigs_links_* -- 2 * from_unitig + from_sign above 2 * to_unitig + to_sign, + = 0, - = 1
def uni_link_word(frm, from_sign, to, to_sign):
    return ((2 * int(frm) + int(from_sign)) << 32) | (2 * int(to) + int(to_sign))


def uni_link_from(w):
    return int(w) >> 33


def uni_link_from_sign(w):
    return (int(w) >> 32) & 1


def uni_link_to(w):
    return (int(w) & 0xFFFFFFFF) >> 1


def uni_link_to_sign(w):
    return int(w) & 1


def uni_link_fields(links):
    """The four columns (from, from_sign, to, to_sign) of an array of link words, as uint32 arrays."""
    w = np.asarray(links, dtype=np.uint64)
    hi, lo = (w >> np.uint64(32)).astype(np.uint32), (w & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return hi >> 1, hi & 1, lo >> 1, lo & 1


# KH_LOC_*: a word of kh_unitigs_locate* -- 2 * unitig + sign above the offset of the k-mer in that unitig, or one of the two specials
LOC_NO_WINDOW = 0xFFFFFFFFFFFFFFFF  # KH_LOC_NO_WINDOW: where kh_profile* writes PROFILE_NO_WINDOW
LOC_ABSENT = 0xFFFFFFFFFFFFFFFE     # KH_LOC_ABSENT: a valid window whose k-mer is not a node of the live unitigs


def loc_word(unitig, sign, offset):
    return ((2 * int(unitig) + int(sign)) << 32) | int(offset)


def loc_unpack(words):
    """The three columns (unitig, sign, offset) of an array of located words, as uint32 arrays, and nothing for the specials:
    their rows hold whatever the bits say -- mask with loc_is_place() first."""
    w = np.asarray(words, dtype=np.uint64)
    hi, lo = (w >> np.uint64(32)).astype(np.uint32), (w & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return hi >> 1, hi & 1, lo


def loc_is_place(words):
    return np.asarray(words, dtype=np.uint64) < np.uint64(LOC_ABSENT)


# KH_RUN_*: the words of a run row of kh_unitigs_paths* -- state (2 * unitig + sign), offset of the run's first window in the unitig,
# first window start and one behind the last, both relative to the record; KH_COV_*: the words per unitig of its coverage array
RUN_WORDS, RUN_STATE, RUN_OFFSET, RUN_QSTART, RUN_QEND = 4, 0, 1, 2, 3
COV_WORDS, COV_WINDOWS, COV_RUNS = 2, 0, 1

# KH_SUP_*: the words of kh_unitigs_link_support* -- pairs of consecutive rows of one record, those without a window start between
# them, those whose word is a link (credited), and the rest
SUP_WORDS, SUP_PAIRS, SUP_ADJACENT, SUP_CREDITED, SUP_MISSING = 4, 0, 1, 2, 3
SUP_NAMES = ("pairs", "adjacent", "credited", "missing")


def link_mirror(words):
    """The mirror of every link word (a << 32) | b: ((b ^ 1) << 32) | (a ^ 1) -- the crossing the reverse-complemented read makes."""
    w = np.asarray(words, dtype=np.uint64)
    one, lo = np.uint64(1), np.uint64(0xFFFFFFFF)
    return (((w & lo) ^ one) << np.uint64(32)) | ((w >> np.uint64(32)) ^ one)

# KH_CLIP_*: the words of kh_clip_tips_into
CLIP_WORDS = 8
CLIP_UNITIGS, CLIP_CANDIDATES, CLIP_CLIPPED, CLIP_CLIPPED_KMERS, CLIP_CLIPPED_COUNT, CLIP_KEPT_KMERS, CLIP_KEPT_COUNT, CLIP_LINKS = range(8)
CLIP_NAMES = ("unitigs", "candidates", "clipped", "clipped_kmers", "clipped_count", "kept_kmers", "kept_count", "links")

# KH_POP_*: the words of kh_pop_bubbles_into
POP_WORDS = 9
POP_UNITIGS, POP_CANDIDATES, POP_POPPED, POP_POPPED_KMERS, POP_POPPED_COUNT, POP_KEPT_KMERS, POP_KEPT_COUNT, POP_LINKS, POP_BUBBLES = range(9)
POP_NAMES = ("unitigs", "candidates", "popped", "popped_kmers", "popped_count", "kept_kmers", "kept_count", "links", "bubbles")

# KH_COMP_*: the words of a component row of kh_unitigs_components* -- its smallest unitig index, its unitigs, the sums of their KMERS
# and COUNT_SUM; KH_CC_*: the words of the call -- components, those of one unitig, the greatest KMERS of a row, the hooking rounds
COMP_WORDS, COMP_FIRST, COMP_UNITIGS, COMP_KMERS, COMP_COUNT_SUM = 4, 0, 1, 2, 3
CC_WORDS, CC_COMPONENTS, CC_SINGLETONS, CC_LARGEST_KMERS, CC_ROUNDS = 4, 0, 1, 2, 3
CC_NAMES = ("components", "singletons", "largest_kmers", "rounds")

# KH_DROP_*: the words of kh_drop_components_into
DROP_WORDS = 9
(DROP_UNITIGS, DROP_COMPONENTS, DROP_DROPPED, DROP_DROPPED_KMERS, DROP_DROPPED_COUNT, DROP_KEPT_KMERS, DROP_KEPT_COUNT, DROP_LINKS,
 DROP_DROPPED_UNITIGS) = range(9)
DROP_NAMES = ("unitigs", "components", "dropped", "dropped_kmers", "dropped_count", "kept_kmers", "kept_count", "links", "dropped_unitigs")


_SET_OPS = {"intersect": SET_INTERSECT, "union": SET_UNION, "subtract": SET_SUBTRACT, "count-subtract": SET_COUNT_SUBTRACT}
_CALCS = {"min": CALC_MIN, "max": CALC_MAX, "sum": CALC_SUM, "left": CALC_LEFT, "right": CALC_RIGHT}


class KhConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_uint32), ("min_quality", C.c_int32),
                ("device", C.c_int32), ("capacity_hint", C.c_uint64), ("stream", C.c_void_p),
                ("flags", C.c_uint32), ("input_mib", C.c_uint32)]


class KhStats(C.Structure):
    _fields_ = [("bases", C.c_uint64), ("kmers", C.c_uint64), ("distinct", C.c_uint64),
                ("table_slots", C.c_uint64), ("grows", C.c_uint64), ("launches", C.c_uint64),
                ("count_kernel_ms", C.c_double), ("h2d_ms", C.c_double), ("part_batches", C.c_uint64),
                ("stage_ms", C.c_double * 8), ("text_scan_ms", C.c_double),
                ("slot_bytes", C.c_uint64)]

class KhUniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


class KhMergeInfo(C.Structure):
    _fields_ = [("route", C.c_uint32), ("pieces", C.c_uint32), ("unit_bytes", C.c_uint32), ("nranks", C.c_uint32),
                ("local_distinct", C.c_uint64), ("sent_units", C.c_uint64), ("recv_units", C.c_uint64),
                ("owned_distinct", C.c_uint64), ("export_ms", C.c_double), ("wait_ms", C.c_double),
                ("merge_ms", C.c_double), ("total_ms", C.c_double),
                ("nranks_seen", C.c_uint32), ("conserved", C.c_uint32), ("sent_count_sum", C.c_uint64),
                ("merged_count_sum", C.c_uint64)]


ROUTES = ("none", "dense", "regions-heads", "regions-packed", "regions", "pairs")  # KH_ROUTE_*
# names of kh_stats.stage_ms[i] (KH_STAGE_* of the header); bench.py maps them to the kernels that ran
STAGES = ("direct", "unused", "level1", "level2_count", "level2", "region", "misc", "grow")
FLAG_TRACE, FLAG_FORCE_DIRECT, FLAG_FORCE_PARTITION, FLAG_CALLER_STREAM, FLAG_DEFER_TEXT_SCAN = 1, 2, 4, 8, 16


# every symbol include/kmerhip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_U64 = C.c_uint64
SYMBOLS = {
    "kh_abi_version": (C.c_int, []),
    "kh_create": (C.c_int, [C.POINTER(_P), C.POINTER(KhConfig)]),
    "kh_destroy": (None, [_P]),
    "kh_reset": (C.c_int, [_P]),
    "kh_push": (C.c_int, [_P, _P, _P, _U64]),
    "kh_push_device": (C.c_int, [_P, _P, _P, _U64]),
    "kh_push_text": (C.c_int, [_P, _P, _U64, C.c_int]),
    "kh_push_text_device": (C.c_int, [_P, _P, _U64, C.c_int]),
    "kh_finish": (C.c_int, [_P, C.POINTER(KhStats)]),
    "kh_result_size": (C.c_int, [_P, _U64, C.POINTER(_U64)]),
    "kh_result_copy": (C.c_int, [_P, _P, _P, _U64, _U64, C.POINTER(_U64)]),
    "kh_result_copy_device": (C.c_int, [_P, _P, _P, _U64, _U64, C.POINTER(_U64)]),
    "kh_result_sorted": (C.c_int, [_P, _P, _P, _U64, _U64, C.POINTER(_U64)]),
    "kh_result_sorted_device": (C.c_int, [_P, _P, _P, _U64, _U64, C.POINTER(_U64)]),
    "kh_result_text_begin": (C.c_int, [_P, C.c_uint32, _U64, C.POINTER(_U64), C.POINTER(_U64)]),
    "kh_result_text_next": (C.c_int, [_P, _P, _U64, C.POINTER(_U64)]),
    "kh_result_text_next_device": (C.c_int, [_P, _P, _U64, C.POINTER(_U64)]),
    "kh_histogram": (C.c_int, [_P, _U64, _P, _P, _U64, C.POINTER(_U64)]),
    "kh_lookup": (C.c_int, [_P, _P, _U64, _P]),
    "kh_profile_device": (C.c_int, [_P, _P, _P, _U64, _P]),
    "kh_profile": (C.c_int, [_P, _P, _P, _U64, _P]),
    "kh_profile_records_device": (C.c_int, [_P, _P, _P, _U64, _P, _U64, C.c_uint32, C.c_uint32, _P]),
    "kh_profile_records": (C.c_int, [_P, _P, _P, _U64, _P, _U64, C.c_uint32, C.c_uint32, _P]),
    "kh_compare": (C.c_int, [_P, _P, _U64, _U64, _P]),
    "kh_combine_into": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _U64, _U64, C.POINTER(_U64)]),
    "kh_graph_stats": (C.c_int, [_P, _U64, _P]),
    "kh_graph_masks_device": (C.c_int, [_P, _P, _U64, _U64, _P]),
    "kh_graph_masks": (C.c_int, [_P, _P, _U64, _U64, _P]),
    "kh_unitigs_begin": (C.c_int, [_P, _U64, _P, _P]),
    "kh_unitigs_copy_device": (C.c_int, [_P, _P, _U64, _P, _U64]),
    "kh_unitigs_copy": (C.c_int, [_P, _P, _U64, _P, _U64]),
    "kh_unitigs_end": (C.c_int, [_P]),
    "kh_unitigs_begin_linked": (C.c_int, [_P, _U64, _P, _P, _P]),
    "kh_unitigs_links_copy_device": (C.c_int, [_P, _P, _U64]),
    "kh_unitigs_links_copy": (C.c_int, [_P, _P, _U64]),
    "kh_unitigs_text_begin": (C.c_int, [_P, C.c_uint32, C.POINTER(_U64)]),
    "kh_unitigs_text_next": (C.c_int, [_P, _P, _U64, C.POINTER(_U64)]),
    "kh_unitigs_text_next_device": (C.c_int, [_P, _P, _U64, C.POINTER(_U64)]),
    "kh_unitigs_locate_device": (C.c_int, [_P, _P, _P, _U64, _P]),
    "kh_unitigs_locate": (C.c_int, [_P, _P, _P, _U64, _P]),
    "kh_unitigs_paths_device": (C.c_int, [_P, _P, _P, _U64, _P, _U64, _P, _P, _U64, _P, C.POINTER(_U64)]),
    "kh_unitigs_paths": (C.c_int, [_P, _P, _P, _U64, _P, _U64, _P, _P, _U64, _P, C.POINTER(_U64)]),
    "kh_unitigs_link_support_device": (C.c_int, [_P, _P, _U64, _P, _U64, _P, _U64, _P]),
    "kh_unitigs_link_support": (C.c_int, [_P, _P, _U64, _P, _U64, _P, _U64, _P]),
    "kh_unitigs_components_device": (C.c_int, [_P, _P, _U64, _P, _U64, _P]),
    "kh_unitigs_components": (C.c_int, [_P, _P, _U64, _P, _U64, _P]),
    "kh_clip_tips_into": (C.c_int, [_P, _P, _U64, _U64, _P]),
    "kh_drop_components_into": (C.c_int, [_P, _P, _U64, _U64, _P]),
    "kh_pop_bubbles_into": (C.c_int, [_P, _P, _U64, _U64, _P]),
    "kh_owner": (C.c_uint32, [_U64, C.c_uint32, C.c_uint32]),
    "kh_set_shard": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "kh_set_region_window": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "kh_region_unit_counts_device": (C.c_int, [_P, C.c_uint32, _P, _U64, _P]),
    "kh_export_regions_device": (C.c_int, [_P, C.c_uint32, _P, _P, _U64, _P, _U64, _P, C.POINTER(_U64)]),
    "kh_merge_regions_device": (C.c_int, [_P, C.c_uint32, _U64, _P, _P, _P]),
    "kh_export_regions_packed_device": (C.c_int, [_P, C.c_uint32, _P, _U64, _P, _U64, _P, C.POINTER(_U64)]),
    "kh_merge_regions_packed_device": (C.c_int, [_P, C.c_uint32, _U64, _P, _P]),
    "kh_export_regions_heads_device": (C.c_int, [_P, C.c_uint32, _P, _U64, _P, _U64, _P, C.POINTER(_U64)]),
    "kh_merge_regions_heads_device": (C.c_int, [_P, C.c_uint32, _U64, _P, _P]),
    "kh_export_dense_device": (C.c_int, [_P, _P, _U64]),
    "kh_merge_dense_device": (C.c_int, [_P, _P, _U64, C.c_uint32, C.c_uint32]),
    "kh_export_by_owner_device": (C.c_int, [_P, C.c_uint32, _P, _P, _U64, _P]),
    "kh_merge_pairs_device": (C.c_int, [_P, _P, _P, _U64]),
    "kh_merge_pairs": (C.c_int, [_P, _P, _P, _U64]),
    "kh_comm_unique_id": (C.c_int, [C.POINTER(KhUniqueId)]),
    "kh_comm_init": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(KhUniqueId)]),
    "kh_merge_across": (C.c_int, [_P, C.POINTER(KhMergeInfo)]),
    "kh_group_create": (C.c_int, [C.POINTER(_P), C.POINTER(KhConfig), C.POINTER(C.c_int32), C.c_uint32]),
    "kh_group_ctx": (_P, [_P, C.c_uint32]),
    "kh_group_size": (C.c_uint32, [_P]),
    "kh_group_merge": (C.c_int, [_P, C.POINTER(KhMergeInfo)]),
    "kh_group_destroy": (None, [_P]),
    "kh_host_alloc": (C.c_int, [C.POINTER(_P), _U64]),
    "kh_host_free": (C.c_int, [_P]),
    "kh_host_register": (C.c_int, [_P, _U64]),
    "kh_host_unregister": (C.c_int, [_P]),
    "kh_pack": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(_U64), C.POINTER(C.c_uint32)]),
    "kh_unpack": (C.c_int, [_U64, C.c_uint32, C.c_char_p]),
    "kh_canonical": (C.c_int, [_U64, C.c_uint32, C.POINTER(_U64), C.POINTER(C.c_int)]),
    "kh_strerror": (C.c_char_p, [C.c_int]),
    "kh_last_error": (C.c_char_p, [_P]),
    "kh_synth_reads_device": (C.c_int, [C.c_int, _P, _U64, _U64, C.c_uint32, _U64, _U64, _P, _P]),
}


class KmerHipError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = lib().kh_strerror(status).decode()
        super().__init__(f"kmerhip error {status}: {msg}" + (f" ({detail})" if detail else ""))


class KmerLengthError(ValueError):
    """Mirror of kmerust::error::KmerLengthError (src/error.rs:86-95)."""

    def __init__(self, k):
        self.k, self.min, self.max = k, 1, 32
        super().__init__(f"k-mer length {k} is out of range: must be between 1 and 32")


_lib = None
ABI_VERSION = 2  # KMERHIP_ABI_VERSION of the include/kmerhip.h this file mirrors (tests/test_abi.py)


def lib():
    """Loads the HIP library; raises ImportError (never falls back) if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C krust_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
        # torch bundles its own libamdhip64.so.7; importing it first makes the dynamic linker
        # resolve our DT_NEEDED entry to that already-loaded copy, so the process holds ONE HIP
        # runtime and tensor.data_ptr() addresses are valid in our kernels.  (torch is plumbing:
        # device memory, streams, torch.distributed.)  Without torch, /opt/rocm/lib is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        if L.kh_abi_version() != ABI_VERSION:  # (the structs below are laid out for this version of include/kmerhip.h)
            raise ImportError(f"{LIB_PATH} speaks ABI version {L.kh_abi_version()}, this binding {ABI_VERSION}: rebuild the library")
        _lib = L
    return _lib


def _addr(a):
    """numpy array / bytes / int address / None -> (address or None, keepalive)."""
    if a is None:
        return None, None
    if isinstance(a, int):
        return a, None
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a
    arr = np.frombuffer(a, dtype=np.uint8)
    return arr.ctypes.data, arr


def _text_format(fmt):
    return {"fasta": TEXT_FASTA, "fastq": TEXT_FASTQ, TEXT_FASTA: TEXT_FASTA, TEXT_FASTQ: TEXT_FASTQ}[fmt]


def _out_format(fmt):
    return {"fasta": KH_OUT_FASTA, "tsv": KH_OUT_TSV, "json": KH_OUT_JSON,
            KH_OUT_FASTA: KH_OUT_FASTA, KH_OUT_TSV: KH_OUT_TSV, KH_OUT_JSON: KH_OUT_JSON}[fmt]


class DeviceCounter:
    """One kh_ctx: a GPU-resident canonical k-mer count table.

    Stands where the reference has `KmerMap` (src/run.rs:491-583): build()/
    build_with_quality() -> push()/push_device(); into_hashmap() -> result()."""

    def __init__(self, k, min_quality=None, capacity_hint=0, device=-1, stream=None, trace=False, path=None, defer_text_scan=False,
                 input_bytes=0):
        """stream: None = the context creates its own non-blocking stream (NOT ordered with torch's streams:
        synchronise buffers you hand over yourself); an integer = launch on that hipStream_t, where 0 is the
        legacy default stream (torch.cuda.current_stream().cuda_stream is usually 0)."""
        if not (1 <= int(k) <= 32):
            raise KmerLengthError(int(k))
        cfg = KhConfig(C.sizeof(KhConfig), int(k), -1 if min_quality is None else int(min_quality),
                       int(device), int(capacity_hint), stream or None,
                       (FLAG_TRACE if trace else 0) | (FLAG_CALLER_STREAM if stream is not None else 0)
                       | (FLAG_DEFER_TEXT_SCAN if defer_text_scan else 0)
                       | {None: 0, "auto": 0, "direct": FLAG_FORCE_DIRECT, "partition": FLAG_FORCE_PARTITION}[path],
                       min(0xFFFFFFFF, (int(input_bytes) + (1 << 20) - 1) >> 20))
        h = _P()
        rc = lib().kh_create(C.byref(h), C.byref(cfg))
        if rc != KH_OK:
            raise KmerHipError(rc)
        self._h = h
        self._owned = True
        self.k = int(k)
        self.min_quality = min_quality

    @classmethod
    def _adopt(cls, handle, k, min_quality):
        """A context that belongs to a DeviceGroup (destroyed with the group, not here)."""
        self = cls.__new__(cls)
        self._h, self._owned, self.k, self.min_quality = _P(handle), False, int(k), min_quality
        return self

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                lib().kh_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != KH_OK:
            raise KmerHipError(rc, lib().kh_last_error(self._h).decode())

    def reset(self):
        self._check(lib().kh_reset(self._h))

    # -- input -------------------------------------------------------------
    def push(self, bases, qual=None):
        """Flat host buffer(s); records separated by >=1 non-ACGT byte."""
        bp, kb = _addr(bases)
        n = kb.size if kb is not None else 0
        qp, kq = _addr(qual)
        if kq is not None and kq.size != n:
            raise ValueError("qual must have the same length as bases")
        self._check(lib().kh_push(self._h, bp, qp, n))

    def push_device(self, d_bases, d_qual, n):
        """Device-resident flat buffers given as integer addresses (e.g. tensor.data_ptr())."""
        self._check(lib().kh_push_device(self._h, d_bases, d_qual, int(n)))

    def push_text(self, text, fmt):
        """Raw FASTA / FASTQ text (whole records) scanned on the device; fmt: "fasta" | "fastq".
        Raises KmerHipError(status=KH_ERR_FORMAT) for layouts the device scanner does not take."""
        tp, kt = _addr(text)
        self._check(lib().kh_push_text(self._h, tp, kt.size if kt is not None else 0, _text_format(fmt)))

    def push_text_device(self, d_text, n, fmt):
        self._check(lib().kh_push_text_device(self._h, d_text, int(n), _text_format(fmt)))

    def finish(self):
        st = KhStats()
        self._check(lib().kh_finish(self._h, C.byref(st)))
        d = {f: getattr(st, f) for f, _ in KhStats._fields_ if f != "stage_ms"}
        d["stage_ms"] = {name: st.stage_ms[i] for i, name in enumerate(STAGES)}
        return d

    # -- output ------------------------------------------------------------
    def result_size(self, min_count=1):
        n = _U64(0)
        self._check(lib().kh_result_size(self._h, int(min_count), C.byref(n)))
        return int(n.value)

    def result(self, min_count=1, sort=True, out=None):
        """(keys, counts) as uint64 arrays; packed canonical keys.  out = (keys, counts) arrays to fill (e.g. views of
        PinnedArray memory: the copy is then one DMA each)."""
        n = self.result_size(min_count)
        if out is not None:
            keys, cnts = out[0][:n], out[1][:n]
            assert keys.size == n and cnts.size == n, "out arrays too small"
        else:
            keys = np.empty(n, dtype=np.uint64)
            cnts = np.empty(n, dtype=np.uint64)
        got = _U64(0)
        self._check(lib().kh_result_copy(self._h, keys.ctypes.data, cnts.ctypes.data, n, int(min_count), C.byref(got)))
        assert got.value == n
        if sort:
            o = np.argsort(keys, kind="stable")
            keys, cnts = keys[o], cnts[o]
        return keys, cnts

    def result_device(self, d_keys, d_counts, cap, min_count=1):
        got = _U64(0)
        self._check(lib().kh_result_copy_device(self._h, d_keys, d_counts, int(cap), int(min_count), C.byref(got)))
        return int(got.value)

    def result_sorted(self, min_count=1):
        """(keys, counts) ascending by key, sorted on the device (kh_result_sorted): the k-mer strings in lexicographic order."""
        n = self.result_size(min_count)
        keys = np.empty(n, dtype=np.uint64)
        cnts = np.empty(n, dtype=np.uint64)
        got = _U64(0)
        self._check(lib().kh_result_sorted(self._h, keys.ctypes.data if n else None, cnts.ctypes.data if n else None, n,
                                           int(min_count), C.byref(got)))
        assert got.value == n
        return keys, cnts

    def result_sorted_device(self, d_keys, d_counts, cap, min_count=1):
        """The same into device arrays of capacity cap (KH_ERR_RANGE, nothing written, when the result is larger)."""
        got = _U64(0)
        self._check(lib().kh_result_sorted_device(self._h, d_keys, d_counts, int(cap), int(min_count), C.byref(got)))
        return int(got.value)

    def as_dict(self, min_count=1):
        k, c = self.result(min_count)
        return dict(zip(k.tolist(), c.tolist()))

    def as_str_dict(self, min_count=1):
        """HashMap<String,u64> of into_hashmap (src/run.rs:573-582)."""
        return {unpack(key, self.k): c for key, c in self.as_dict(min_count).items()}

    # -- output as text, formatted on the device -----------------------------
    def result_text_begin(self, format, min_count=1, sorted=False):
        """Starts (or restarts) the text stream of the records with count >= min_count; format: "fasta" | "tsv" | "json".
        sorted: the records come in ascending key order (KH_OUT_SORTED) instead of table-slot order.
        Returns (n_records, n_bytes) of the whole stream."""
        nr, nb = _U64(0), _U64(0)
        fmt = _out_format(format) | (KH_OUT_SORTED if sorted else 0)
        self._check(lib().kh_result_text_begin(self._h, fmt, int(min_count), C.byref(nr), C.byref(nb)))
        return int(nr.value), int(nb.value)

    def result_text_next(self, buf, cap=None):
        """The next piece (whole records, at most cap bytes) into `buf`: a writable numpy uint8 array (pageable, or a
        PinnedArray's) or an integer host address with `cap`.  Returns the bytes written; 0 = the stream has ended.
        Raises KmerHipError with status KH_ERR_RANGE when cap is smaller than the next record (nothing is consumed)."""
        if isinstance(buf, np.ndarray):
            assert buf.dtype == np.uint8 and buf.flags.c_contiguous and buf.flags.writeable
            addr, cap = buf.ctypes.data, buf.size if cap is None else min(int(cap), buf.size)
        else:
            addr, cap = int(buf), int(cap)
        n = _U64(0)
        self._check(lib().kh_result_text_next(self._h, addr, cap, C.byref(n)))
        return int(n.value)

    def result_text(self, format, min_count=1, piece_bytes=8 << 20, sorted=False):
        """Generator over the table as text: `bytes` pieces of at most piece_bytes that end at record ends and whose
        concatenation is the whole document (the reference's output_counts, src/run.rs:441-486, formatted on the device)."""
        self.result_text_begin(format, min_count, sorted=sorted)
        buf = np.empty(max(int(piece_bytes), 1), dtype=np.uint8)
        while True:
            n = self.result_text_next(buf)
            if n == 0:
                return
            yield buf[:n].tobytes()

    def result_text_device(self, out, cap=None, format=None, min_count=1):
        """The next piece into DEVICE memory: `out` is a uint8 tensor on this context's device, or an integer device address
        with `cap`.  format given: the stream is (re)started first.  Returns the bytes written; 0 = the stream has ended."""
        if format is not None:
            self.result_text_begin(format, min_count)
        if isinstance(out, int):
            addr, cap = out, int(cap)
        else:
            addr, cap = out.data_ptr(), out.numel() * out.element_size() if cap is None else int(cap)
        n = _U64(0)
        self._check(lib().kh_result_text_next_device(self._h, addr, cap, C.byref(n)))
        return int(n.value)

    def histogram(self, min_count=1):
        cap = 1 << 12
        while True:
            cnt = np.empty(cap, dtype=np.uint64)
            frq = np.empty(cap, dtype=np.uint64)
            n = _U64(0)
            rc = lib().kh_histogram(self._h, int(min_count), cnt.ctypes.data, frq.ctypes.data, cap, C.byref(n))
            if rc == KH_ERR_RANGE:
                cap *= 16
                continue
            self._check(rc)
            return list(zip(cnt[: n.value].tolist(), frq[: n.value].tolist()))

    def lookup(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(keys.size, dtype=np.uint64)
        self._check(lib().kh_lookup(self._h, keys.ctypes.data, keys.size, out.ctypes.data))
        return out

    def profile(self, bases, qual=None, out=None):
        """Per-base abundance: a uint32 array with one entry per byte of the flat buffer `bases` (records separated by a byte
        outside ACGTacgt; `qual` masks as in counting) -- entry i is the table's count of the canonical k-mer of bytes
        i .. i+k-1, saturated at 0xFFFFFFFE, 0 when the table does not hold it, PROFILE_NO_WINDOW where counting would see no
        window.  Host memory, pageable or a PinnedArray's; out = a uint32 array to fill (e.g. a PinnedArray's: no bounce)."""
        bp, kb = _addr(bases)
        n = kb.size if kb is not None else 0
        qp, kq = _addr(qual)
        if kq is not None and kq.size != n:
            raise ValueError("qual must have the same length as bases")
        if out is None:
            out = np.empty(n, dtype=np.uint32)
        assert out.dtype == np.uint32 and out.flags.c_contiguous and out.flags.writeable and out.size >= n
        self._check(lib().kh_profile(self._h, bp, qp, n, out.ctypes.data))
        return out[:n]

    def profile_device(self, d_bases, d_qual, n, d_out):
        """The same on device memory: integer addresses (e.g. tensor.data_ptr()) of n bases, n quality bytes or None, and n
        uint32 entries to fill, or torch tensors on this context's device.  Returns when d_out is complete."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        self._check(lib().kh_profile_device(self._h, ptr(d_bases), ptr(d_qual), int(n), ptr(d_out)))

    def profile_records(self, bases, rec_start, qual=None, lo=1, hi=0xFFFFFFFE, out=None):
        """The profile of `bases` reduced per record on the device: rec_start holds nrec + 1 ascending offsets into the flat
        buffer (record r owns the window starts rec_start[r] .. rec_start[r+1]; the last offset <= len(bases)).  Returns an
        (nrec, 8) uint32 array, columns REC_WINDOWS .. REC_FIRST_LOW: windows, present (count > 0), in_range (lo <= count <= hi),
        min, max, the sum's low and high word, and the offset of the first window with a count < lo (0xFFFFFFFF: none)."""
        bp, kb = _addr(bases)
        n = kb.size if kb is not None else 0
        qp, kq = _addr(qual)
        if kq is not None and kq.size != n:
            raise ValueError("qual must have the same length as bases")
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        if rs.ndim != 1 or rs.size < 1:
            raise ValueError("rec_start needs nrec + 1 offsets")
        nrec = rs.size - 1
        if out is None:
            out = np.empty((nrec, REC_WORDS), dtype=np.uint32)
        assert out.dtype == np.uint32 and out.flags.c_contiguous and out.flags.writeable and out.size >= nrec * REC_WORDS
        self._check(lib().kh_profile_records(self._h, bp, qp, n, rs.ctypes.data, nrec, int(lo), int(hi), out.ctypes.data))
        return out.reshape(-1)[:nrec * REC_WORDS].reshape(nrec, REC_WORDS)

    def profile_records_device(self, d_bases, d_qual, n, d_rec_start, nrec, d_rows, lo=1, hi=0xFFFFFFFE):
        """The same on device memory: integer addresses or torch tensors of n bases, n quality bytes or None, nrec + 1 uint64
        offsets and nrec * 8 uint32 words to fill.  The offsets are the caller's contract (not checked).  Returns when d_rows
        is complete."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        self._check(lib().kh_profile_records_device(self._h, ptr(d_bases), ptr(d_qual), int(n), ptr(d_rec_start), int(nrec), int(lo),
                                                    int(hi), ptr(d_rows)))

    # -- two tables against each other ---------------------------------------
    def compare(self, other, min_a=1, min_b=1):
        """kh_compare of this table (a) and `other` (b), both only read: a dict of the eight words -- distinct_a, distinct_b,
        shared, sum_a, sum_b, shared_sum_a, shared_sum_b, sum_min -- over the keys with a count >= max(min_a, 1) here and
        >= max(min_b, 1) there.  Jaccard = shared / (distinct_a + distinct_b - shared), containment = shared / distinct_a,
        Bray-Curtis = 1 - 2 sum_min / (sum_a + sum_b)."""
        out = np.zeros(CMP_WORDS, dtype=np.uint64)
        self._check(lib().kh_compare(self._h, other._h, int(min_a), int(min_b), out.ctypes.data))
        return dict(zip(CMP_NAMES, (int(x) for x in out)))

    def combine_into(self, a, b, op, calc=CALC_SUM, min_a=1, min_b=1):
        """kh_combine_into: adds the pairs of the set operation `op` ("intersect" | "union" | "subtract" | "count-subtract" or
        SET_*) of the tables a and b to THIS table (count[key] += c); calc ("min" | "max" | "sum" | "left" | "right" or CALC_*)
        is the count of a key both hold.  a and b are only read; this table must be neither.  Returns the number of pairs."""
        n = _U64(0)
        self._check(lib().kh_combine_into(self._h, a._h, b._h, int(_SET_OPS.get(op, op)), int(_CALCS.get(calc, calc)), int(min_a),
                                          int(min_b), C.byref(n)))
        return int(n.value)

    # -- the table against itself: de Bruijn graph degrees --------------------
    def graph_stats(self, min_count=1):
        """kh_graph_stats: a uint64 array of GRAPH_WORDS words over the node set S = the keys with a count >= max(min_count, 1) --
        [m] for m < 256 = the nodes whose neighbour mask is m, [GRAPH_NODES] = |S|, [GRAPH_KMERS] = the sum of their counts."""
        out = np.zeros(GRAPH_WORDS, dtype=np.uint64)
        self._check(lib().kh_graph_stats(self._h, int(min_count), out.ctypes.data))
        return out

    def graph_masks(self, keys, min_count=1):
        """kh_graph_masks: a uint8 array, one mask per packed canonical key -- bit c (GRAPH_RIGHT) set iff the right neighbour
        by letter c is in S, bit 4 + c (GRAPH_LEFT) iff the left one is; 0 for a word that is no canonical key of this k.  The
        keys need not be in S themselves.  With the keys of result() / result_sorted() the masks line up with those pairs."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(keys.size, dtype=np.uint8)
        self._check(lib().kh_graph_masks(self._h, keys.ctypes.data if keys.size else None, keys.size, int(min_count),
                                         out.ctypes.data if keys.size else None))
        return out

    def graph_masks_device(self, d_keys, n, d_masks, min_count=1):
        """The same on device memory: integer addresses or torch tensors of n uint64 keys and n bytes to fill, both at any
        alignment.  Returns when d_masks is complete."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        self._check(lib().kh_graph_masks_device(self._h, ptr(d_keys), int(n), int(min_count), ptr(d_masks)))

    # -- unitigs: the compacted de Bruijn graph ------------------------------
    def unitigs_begin(self, min_count=1):
        """kh_unitigs_begin: builds the unitigs of the node set S = the keys with a count >= max(min_count, 1) into device memory
        of the context's own; returns (n_unitigs, n_bases).  unitigs_copy* fetch them, unitigs_end releases them."""
        nu, nb = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().kh_unitigs_begin(self._h, int(min_count), C.byref(nu), C.byref(nb)))
        return int(nu.value), int(nb.value)

    def unitigs_copy(self, n_unitigs, n_bases):
        """kh_unitigs_copy into fresh arrays: rows (n_unitigs, UNI_WORDS) uint64 -- START, KMERS, COUNT_SUM, FLAGS -- and the
        bases (uint8, ASCII ACGT, unitig after unitig; a unitig of L k-mers has L + k - 1 of them)."""
        rows = np.zeros((int(n_unitigs), UNI_WORDS), dtype=np.uint64)
        bases = np.zeros(int(n_bases), dtype=np.uint8)
        self._check(lib().kh_unitigs_copy(self._h, rows.ctypes.data if rows.size else None, rows.shape[0],
                                          bases.ctypes.data if bases.size else None, bases.size))
        return rows, bases

    def unitigs_copy_device(self, d_rows, row_cap, d_bases, base_cap):
        """The same into device memory: integer addresses or torch tensors (rows 8-byte aligned, bases at any alignment) with
        room for row_cap rows and base_cap bases.  Returns when both are complete."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        self._check(lib().kh_unitigs_copy_device(self._h, ptr(d_rows), int(row_cap), ptr(d_bases), int(base_cap)))

    def unitigs_end(self):
        self._check(lib().kh_unitigs_end(self._h))

    def unitigs(self, min_count=1):
        """(rows, bases) of the unitigs of S, in ascending key order of their first nodes: begin, copy, end."""
        nu, nb = self.unitigs_begin(min_count)
        try:
            return self.unitigs_copy(nu, nb)
        finally:
            self.unitigs_end()

    # -- the live unitigs as text, formatted on the device --------------------
    def unitigs_text_begin(self, format):
        """kh_unitigs_text_begin: starts (or restarts) the text stream of the live unitigs; format: "fasta" (what `kmerust unitigs`
        prints) | "gfa" (what `kmerust gfa` prints; needs unitigs_begin_linked) or a KH_UNI_TEXT_* value.  Returns the document's
        length in bytes."""
        nb = _U64(0)
        fmt = {"fasta": KH_UNI_TEXT_FASTA, "gfa": KH_UNI_TEXT_GFA}.get(format, format)
        self._check(lib().kh_unitigs_text_begin(self._h, int(fmt), C.byref(nb)))
        return int(nb.value)

    def unitigs_text_next(self, buf, cap=None):
        """The next piece -- a byte range, min(cap, bytes left) long -- into `buf`: a writable numpy uint8 array (pageable, or a
        PinnedArray's) or an integer host address with `cap`.  Returns the bytes written; 0 = the stream has ended."""
        if isinstance(buf, np.ndarray):
            assert buf.dtype == np.uint8 and buf.flags.c_contiguous and buf.flags.writeable
            addr, cap = buf.ctypes.data, buf.size if cap is None else min(int(cap), buf.size)
        else:
            addr, cap = int(buf), int(cap)
        n = _U64(0)
        self._check(lib().kh_unitigs_text_next(self._h, addr, cap, C.byref(n)))
        return int(n.value)

    def unitigs_text_next_device(self, out, cap=None):
        """The next piece into DEVICE memory at any alignment: `out` is a uint8 tensor on this context's device, or an integer
        device address with `cap`.  Returns the bytes written; 0 = the stream has ended."""
        if isinstance(out, int):
            addr, cap = out, int(cap)
        else:
            addr, cap = out.data_ptr(), out.numel() * out.element_size() if cap is None else int(cap)
        n = _U64(0)
        self._check(lib().kh_unitigs_text_next_device(self._h, addr, cap, C.byref(n)))
        return int(n.value)

    def unitigs_text(self, format, piece_bytes=8 << 20):
        """The whole document of the live unitigs as `bytes`: begin, then pieces of piece_bytes until the stream has ended."""
        total = self.unitigs_text_begin(format)
        buf = np.empty(max(int(piece_bytes), 1), dtype=np.uint8)
        out = bytearray()
        while True:
            n = self.unitigs_text_next(buf)
            if n == 0:
                break
            out += buf[:n].tobytes()
        assert len(out) == total, (len(out), total)
        return bytes(out)

    # -- links between unitigs: the edges of the compacted graph -------------
    def unitigs_begin_linked(self, min_count=1):
        """kh_unitigs_begin_linked: unitigs_begin plus the links between the unitigs' ends; returns (n_unitigs, n_bases, n_links).
        unitigs_copy* and unitigs_links_copy* fetch them, unitigs_end releases all of it."""
        nu, nb, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(lib().kh_unitigs_begin_linked(self._h, int(min_count), C.byref(nu), C.byref(nb), C.byref(nl)))
        self._n_links = int(nl.value)   # (what unitigs_link_support sizes a fresh array with)
        self._n_unitigs = int(nu.value)  # (and unitigs_components)
        return int(nu.value), int(nb.value), int(nl.value)

    def unitigs_links_copy(self, n_links):
        """kh_unitigs_links_copy into a fresh uint64 array: one word per link, ascending (uni_link_* take a word apart)."""
        links = np.zeros(int(n_links), dtype=np.uint64)
        self._check(lib().kh_unitigs_links_copy(self._h, links.ctypes.data if links.size else None, links.size))
        return links

    def unitigs_links_copy_device(self, d_links, cap):
        """The same into device memory: an integer address or a torch tensor, 8-byte aligned, with room for cap words.  Returns
        when it is complete."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        self._check(lib().kh_unitigs_links_copy_device(self._h, ptr(d_links), int(cap)))

    def unitigs_linked(self, min_count=1):
        """(rows, bases, links) of the unitigs of S and the links between their ends: begin, copy, end."""
        nu, nb, nl = self.unitigs_begin_linked(min_count)
        try:
            rows, bases = self.unitigs_copy(nu, nb)
            return rows, bases, self.unitigs_links_copy(nl)
        finally:
            self.unitigs_end()

    # -- new sequences located on the live unitigs -----------------------------
    def unitigs_locate(self, bases, qual=None, out=None):
        """kh_unitigs_locate: a uint64 array with one word per byte of the flat buffer `bases` (records separated by a byte outside
        ACGTacgt; `qual` masks as in counting) -- entry i is LOC_NO_WINDOW where profile() says PROFILE_NO_WINDOW, LOC_ABSENT for a
        k-mer that is no node of the live unitigs, else the place of the k-mer of bytes i .. i+k-1: loc_unpack() gives unitig, sign
        and offset.  Needs unitigs_begin / unitigs_begin_linked.  Host memory, pageable or a PinnedArray's; out = a uint64 array to fill."""
        bp, kb = _addr(bases)
        n = kb.size if kb is not None else 0
        qp, kq = _addr(qual)
        if kq is not None and kq.size != n:
            raise ValueError("qual must have the same length as bases")
        if out is None:
            out = np.empty(n, dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.flags.writeable and out.size >= n
        self._check(lib().kh_unitigs_locate(self._h, bp, qp, n, out.ctypes.data))
        return out[:n]

    def unitigs_locate_device(self, d_bases, d_qual, n, d_out):
        """The same on device memory: integer addresses (e.g. tensor.data_ptr()) of n bases, n quality bytes or None, and n uint64
        words to fill (8-byte aligned), or torch tensors on this context's device.  Returns when d_out is complete."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        self._check(lib().kh_unitigs_locate_device(self._h, ptr(d_bases), ptr(d_qual), int(n), ptr(d_out)))

    # -- the same walk as run-compressed paths ---------------------------------
    def unitigs_paths(self, bases, rec_start, qual=None, cover=None, run_cap=None):
        """kh_unitigs_paths: the words of unitigs_locate(bases, qual) folded on the device into runs.  rec_start holds nrec + 1
        ascending offsets into the flat buffer (record r owns the window starts rec_start[r] .. rec_start[r+1]; the last offset
        <= len(bases)).  Returns (run_start, runs): nrec + 1 uint64 CSR offsets and an (n_runs, 4) uint32 array, columns RUN_STATE
        (2 * unitig + sign), RUN_OFFSET (of the run's first window in the unitig), RUN_QSTART and RUN_QEND (window starts relative
        to the record) -- the runs of record r are rows run_start[r] .. run_start[r+1].  cover: a uint64 array of n_unitigs *
        COV_WORDS words that the call adds the windows and the runs per unitig to.  run_cap=None sizes with a first call
        (run_cap 0); with a run_cap that is too small the call raises KmerHipError(KH_ERR_RANGE) and adds nothing to cover."""
        bp, kb = _addr(bases)
        n = kb.size if kb is not None else 0
        qp, kq = _addr(qual)
        if kq is not None and kq.size != n:
            raise ValueError("qual must have the same length as bases")
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        if rs.ndim != 1 or rs.size < 1:
            raise ValueError("rec_start needs nrec + 1 offsets")
        nrec = rs.size - 1
        if cover is not None:
            assert cover.dtype == np.uint64 and cover.flags.c_contiguous and cover.flags.writeable
        cp = None if cover is None else cover.ctypes.data
        run_start = np.zeros(nrec + 1, dtype=np.uint64)
        total = _U64(0)
        if run_cap is None:
            rc = lib().kh_unitigs_paths(self._h, bp, qp, n, rs.ctypes.data, nrec, run_start.ctypes.data, None, 0, None, C.byref(total))
            if rc != KH_ERR_RANGE:
                self._check(rc)
                if cover is None:
                    return run_start, np.empty((0, RUN_WORDS), dtype=np.uint32)
            run_cap = total.value
        runs = np.empty((int(run_cap), RUN_WORDS), dtype=np.uint32)
        self._check(lib().kh_unitigs_paths(self._h, bp, qp, n, rs.ctypes.data, nrec, run_start.ctypes.data,
                                           runs.ctypes.data if run_cap else None, int(run_cap), cp, C.byref(total)))
        return run_start, runs[:total.value]

    def unitigs_paths_device(self, d_bases, d_qual, n, d_rec_start, nrec, d_run_start, d_runs, run_cap, d_cover=None):
        """The same on device memory: integer addresses or torch tensors of n bases, n quality bytes or None, nrec + 1 uint64
        offsets (the caller's contract, not checked), nrec + 1 uint64 words and run_cap * 4 uint32 words to fill, and n_unitigs * 2
        uint64 words to add to, or None.  Returns (status, n_runs) with status KH_OK or KH_ERR_RANGE -- run_cap was too small:
        n_runs and d_run_start are complete, size d_runs and call again --, and raises for every other status.  Returns when the
        outputs are complete."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        total = _U64(0)
        rc = lib().kh_unitigs_paths_device(self._h, ptr(d_bases), ptr(d_qual), int(n), ptr(d_rec_start), int(nrec), ptr(d_run_start),
                                           ptr(d_runs), int(run_cap), ptr(d_cover), C.byref(total))
        if rc != KH_ERR_RANGE:
            self._check(rc)
        return rc, total.value

    # -- read support per link -------------------------------------------------
    def unitigs_link_support(self, run_start, runs, support=None):
        """kh_unitigs_link_support: how many records walk every link of unitigs_begin_linked.  run_start and runs are what
        unitigs_paths returned.  Two consecutive rows of a record with QEND == the next QSTART are a crossing; if its word
        (STATE_i << 32) | STATE_i+1 is link number l of unitigs_links_copy, support[l] += 1.  support: a uint64 array of at least
        n_links counters that the call ADDS to (a caller streams batches into it), or None for a fresh one of the n_links of this
        object's last unitigs_begin_linked.  Returns (support, stats), stats a dict of this call's pairs, adjacent, credited and
        missing (link_mirror gives the word the reverse-complemented read credits)."""
        rs = np.ascontiguousarray(run_start, dtype=np.uint64)
        rows = np.ascontiguousarray(runs, dtype=np.uint32).reshape(-1, RUN_WORDS)
        if rs.ndim != 1 or rs.size < 1:
            raise ValueError("run_start needs nrec + 1 offsets")
        if support is None:
            if getattr(self, "_n_links", None) is None:
                raise ValueError("support=None needs the n_links of a unitigs_begin_linked made through this object")
            support = np.zeros(self._n_links, dtype=np.uint64)
        assert support.dtype == np.uint64 and support.ndim == 1 and support.flags.c_contiguous and support.flags.writeable
        out = np.zeros(SUP_WORDS, dtype=np.uint64)
        self._check(lib().kh_unitigs_link_support(self._h, rs.ctypes.data, rs.size - 1, rows.ctypes.data if rows.size else None, rows.shape[0],
                                                  support.ctypes.data if support.size else None, support.size, out.ctypes.data))
        return support, dict(zip(SUP_NAMES, (int(x) for x in out)))

    def unitigs_link_support_device(self, d_run_start, nrec, d_runs, n_runs, d_support, cap):
        """The same on device memory: integer addresses or torch tensors of nrec + 1 uint64 offsets and n_runs * 4 uint32 words (the
        caller's contract, not checked: what unitigs_paths_device left there) and cap >= n_links uint64 counters to add to.  Returns
        the stats dict when d_support is complete."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        out = np.zeros(SUP_WORDS, dtype=np.uint64)
        self._check(lib().kh_unitigs_link_support_device(self._h, ptr(d_run_start), int(nrec), ptr(d_runs), int(n_runs), ptr(d_support), int(cap),
                                                         out.ctypes.data))
        return dict(zip(SUP_NAMES, (int(x) for x in out)))

    # -- connected components of the unitig graph -------------------------------
    def unitigs_components(self, n_unitigs=None):
        """kh_unitigs_components: which unitigs of unitigs_begin_linked hang together through links (signs and direction ignored,
        self links join nothing).  Returns (comp, rows, stats): comp a uint32 array with the dense component id of every unitig
        (ids ascend with the component's smallest unitig index), rows a (components, 4) uint64 array with the columns COMP_FIRST,
        COMP_UNITIGS, COMP_KMERS and COMP_COUNT_SUM, stats a dict of components, singletons, largest_kmers and rounds.  n_unitigs:
        None for the count of this object's last unitigs_begin_linked.  The first call after a begin builds the labels on the
        device; later ones copy."""
        if n_unitigs is None:
            if getattr(self, "_n_unitigs", None) is None:
                raise ValueError("n_unitigs=None needs a unitigs_begin_linked made through this object")
            n_unitigs = self._n_unitigs
        out = np.zeros(CC_WORDS, dtype=np.uint64)
        self._check(lib().kh_unitigs_components(self._h, None, 0, None, 0, out.ctypes.data))  # (sizes the rows)
        comp = np.zeros(int(n_unitigs), dtype=np.uint32)
        rows = np.zeros((int(out[CC_COMPONENTS]), COMP_WORDS), dtype=np.uint64)
        self._check(lib().kh_unitigs_components(self._h, comp.ctypes.data if comp.size else None, comp.size,
                                                rows.ctypes.data if rows.size else None, rows.shape[0], out.ctypes.data))
        return comp, rows, dict(zip(CC_NAMES, (int(x) for x in out)))

    def unitigs_components_device(self, d_comp, comp_cap, d_rows, row_cap):
        """The same into device memory: integer addresses or torch tensors of comp_cap uint32 words and row_cap * 4 uint64 words,
        either None with a cap of 0 (not wanted).  Returns (status, stats) with status KH_OK or KH_ERR_RANGE -- a cap was too
        small: stats is complete and nothing was written, size the arrays and call again --, and raises for every other status."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        out = np.zeros(CC_WORDS, dtype=np.uint64)
        rc = lib().kh_unitigs_components_device(self._h, ptr(d_comp), int(comp_cap), ptr(d_rows), int(row_cap), out.ctypes.data)
        if rc != KH_ERR_RANGE:
            self._check(rc)
        return rc, dict(zip(CC_NAMES, (int(x) for x in out)))

    # -- dropping small components: one round over the compacted graph ----------
    def drop_components_into(self, src, min_count=1, min_kmers=None):
        """kh_drop_components_into: the k-mers of every unitig of `src`'s compacted graph at min_count whose connected component
        holds at least min_kmers k-mers (None: 2 * k) are added to THIS table with their counts from src (count[key] += c); smaller
        components -- the isolated debris clipping and popping cannot touch -- are left out.  0 or 1 drops nothing.  src's table
        is only read, unitigs it had begun are released; this table must not be src.  Returns the nine words as a dict: unitigs,
        components, dropped, dropped_kmers, dropped_count, kept_kmers, kept_count, links, dropped_unitigs."""
        out = np.zeros(DROP_WORDS, dtype=np.uint64)
        mk = 2 * self.k if min_kmers is None else int(min_kmers)
        self._check(lib().kh_drop_components_into(self._h, src._h, int(min_count), mk, out.ctypes.data))
        return dict(zip(DROP_NAMES, (int(x) for x in out)))

    # -- tip clipping: one round over the compacted graph ---------------------
    def clip_tips_into(self, src, min_count=1, max_kmers=None):
        """kh_clip_tips_into: one round of tip clipping of `src`'s compacted graph at min_count -- the k-mers of every surviving
        unitig are added to THIS table with their counts from src (count[key] += c).  A dead-end unitig of at most max_kmers
        k-mers (None: k) is clipped when at every link out of its attached end a rival beats it (include/kmerhip.h).  src's
        table is only read, unitigs it had begun are released; this table must not be src.  Returns the eight words as a dict:
        unitigs, candidates, clipped, clipped_kmers, clipped_count, kept_kmers, kept_count, links."""
        out = np.zeros(CLIP_WORDS, dtype=np.uint64)
        mk = self.k if max_kmers is None else int(max_kmers)
        self._check(lib().kh_clip_tips_into(self._h, src._h, int(min_count), mk, out.ctypes.data))
        return dict(zip(CLIP_NAMES, (int(x) for x in out)))

    # -- bubble popping: one round over the compacted graph --------------------
    def pop_bubbles_into(self, src, min_count=1, max_kmers=None):
        """kh_pop_bubbles_into: one round of bubble popping of `src`'s compacted graph at min_count -- the k-mers of every surviving
        unitig are added to THIS table with their counts from src (count[key] += c).  Non-circular unitigs of at most max_kmers
        k-mers (None: 2 * k; the branch of a SNP has k) with one link out of each end are parallel when the two ends enter the
        same pair of states; of each such class only the one with the greatest mean count stays (then the most k-mers, then the
        smallest index: include/kmerhip.h).  src's table is only read, unitigs it had begun are released; this table must not be
        src.  Returns the nine words as a dict: unitigs, candidates, popped, popped_kmers, popped_count, kept_kmers, kept_count,
        links, bubbles."""
        out = np.zeros(POP_WORDS, dtype=np.uint64)
        mk = 2 * self.k if max_kmers is None else int(max_kmers)
        self._check(lib().kh_pop_bubbles_into(self._h, src._h, int(min_count), mk, out.ctypes.data))
        return dict(zip(POP_NAMES, (int(x) for x in out)))

    # -- multi-GPU merge ---------------------------------------------------
    def comm_init(self, nranks, rank, unique_id):
        """Joins the RCCL communicator named by `unique_id` (128 bytes from comm_unique_id() of rank 0) as
        `rank` of `nranks`: collective, blocks until every rank has called it."""
        uid = KhUniqueId()
        C.memmove(C.byref(uid), bytes(unique_id), 128)
        self._check(lib().kh_comm_init(self._h, int(nranks), int(rank), C.byref(uid)))

    def merge_across(self):
        """kh_merge_across: the whole exchange inside the library (collective over the communicator's ranks).
        Afterwards this context holds the keys with owner(key, k, nranks) == rank.  Returns the merge info."""
        info = KhMergeInfo()
        self._check(lib().kh_merge_across(self._h, C.byref(info)))
        return merge_info_dict(info)

    def export_by_owner_device(self, nparts, d_keys, d_counts, cap):
        parts = np.zeros(nparts, dtype=np.uint64)
        self._check(lib().kh_export_by_owner_device(self._h, int(nparts), d_keys, d_counts, int(cap), parts.ctypes.data))
        return parts

    def set_shard(self, index, count):
        """Make the (empty) table shard `index` of `count` (power of two) by hash range."""
        self._check(lib().kh_set_shard(self._h, int(index), int(count)))

    def set_region_window(self, piece=0, npieces=1):
        """The next region-ordered exports / merges cover piece `piece` of `npieces` of every owner's
        region range (kh_set_region_window); (0, 1) = everything."""
        self._check(lib().kh_set_region_window(self._h, int(piece), int(npieces)))

    def region_unit_counts_device(self, unit_bytes, d_region_counts, region_cap):
        """Exchange units (4: heads, 8: packed pairs, 16: pairs) per region of the whole table; returns
        the number of table regions, or None where the matching export would not be representable."""
        nreg = _U64(0)
        rc = lib().kh_region_unit_counts_device(self._h, int(unit_bytes), C.c_void_p(int(d_region_counts)), int(region_cap), C.byref(nreg))
        if rc == KH_ERR_RANGE:
            return None
        self._check(rc)
        return int(nreg.value)

    def export_regions_device(self, nparts, d_keys, d_counts, cap, d_region_counts, region_cap):
        """Live pairs in region order (grouped by owner) + per-region live counts.
        Returns (pairs per owner as uint64 array, number of table regions)."""
        parts = np.zeros(nparts, dtype=np.uint64)
        nreg = _U64(0)
        self._check(lib().kh_export_regions_device(self._h, int(nparts), d_keys, d_counts, int(cap), d_region_counts,
                                                   int(region_cap), parts.ctypes.data, C.byref(nreg)))
        return parts, int(nreg.value)

    def merge_regions_device(self, sender_regions, d_keys, d_counts, d_region_counts):
        """d_keys / d_counts / d_region_counts: one device address per sender."""
        n = len(d_keys)
        assert len(d_counts) == n and len(d_region_counts) == n
        arr = lambda xs: (_P * n)(*[_P(int(x)) for x in xs])
        ak, ac, ar = arr(d_keys), arr(d_counts), arr(d_region_counts)
        self._check(lib().kh_merge_regions_device(self._h, n, int(sender_regions), ak, ac, ar))

    def export_regions_packed_device(self, nparts, d_pairs, cap, d_region_counts, region_cap):
        """Packed export (one u64 per pair).  Returns (parts, regions), or None when the table is not
        representable in the packed form (large k for the table size, or a count >= 2^32)."""
        parts = np.zeros(nparts, dtype=np.uint64)
        nreg = _U64(0)
        rc = lib().kh_export_regions_packed_device(self._h, int(nparts), d_pairs, int(cap), d_region_counts,
                                                   int(region_cap), parts.ctypes.data, C.byref(nreg))
        if rc == KH_ERR_RANGE:
            return None
        self._check(rc)
        return parts, int(nreg.value)

    def export_regions_heads_device(self, nparts, d_heads, cap, d_region_counts, region_cap):
        """32-bit heads export.  Returns (heads per owner, regions), or None when not representable
        (k too large for the table size, a very large count, or more than `cap` heads)."""
        parts = np.zeros(nparts, dtype=np.uint64)
        nreg = _U64(0)
        rc = lib().kh_export_regions_heads_device(self._h, int(nparts), d_heads, int(cap), d_region_counts,
                                                  int(region_cap), parts.ctypes.data, C.byref(nreg))
        if rc == KH_ERR_RANGE:
            return None
        self._check(rc)
        return parts, int(nreg.value)

    def merge_regions_heads_device(self, sender_regions, d_heads, d_region_counts):
        n = len(d_heads)
        assert len(d_region_counts) == n
        arr = lambda xs: (_P * n)(*[_P(int(x)) for x in xs])
        ah, ar = arr(d_heads), arr(d_region_counts)
        self._check(lib().kh_merge_regions_heads_device(self._h, n, int(sender_regions), ah, ar))

    def merge_regions_packed_device(self, sender_regions, d_pairs, d_region_counts):
        n = len(d_pairs)
        assert len(d_region_counts) == n
        arr = lambda xs: (_P * n)(*[_P(int(x)) for x in xs])
        ap, ar = arr(d_pairs), arr(d_region_counts)
        self._check(lib().kh_merge_regions_packed_device(self._h, n, int(sender_regions), ap, ar))

    def export_dense_device(self, d_dense, n_entries):
        """Small k (2k <= 26): d_dense[key] = count over the whole 4^k key space."""
        self._check(lib().kh_export_dense_device(self._h, d_dense, int(n_entries)))

    def merge_dense_device(self, d_dense, n_entries, owner, nparts):
        self._check(lib().kh_merge_dense_device(self._h, d_dense, int(n_entries), int(owner), int(nparts)))

    def merge_pairs_device(self, d_keys, d_counts, n):
        self._check(lib().kh_merge_pairs_device(self._h, d_keys, d_counts, int(n)))

    def merge_pairs(self, keys, counts):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        assert keys.size == counts.size
        self._check(lib().kh_merge_pairs(self._h, keys.ctypes.data, counts.ctypes.data, keys.size))


def merge_info_dict(info):
    d = {f: getattr(info, f) for f, _ in KhMergeInfo._fields_}
    d["path"] = ROUTES[info.route] + (f"-x{info.pieces}" if info.pieces > 1 else "")
    return d


def comm_unique_id():
    """128 opaque bytes (an ncclUniqueId) that name a new communicator; rank 0 makes it, every rank gets a copy."""
    uid = KhUniqueId()
    rc = lib().kh_comm_unique_id(C.byref(uid))
    if rc != KH_OK:
        raise KmerHipError(rc)
    return bytes(C.string_at(C.byref(uid), 128))


class DeviceGroup:
    """kh_group: one context per listed device inside ONE process, one host thread per context for the merge.
    Distinct devices exchange over RCCL; a device listed twice (1-GPU test boxes) makes the group exchange by
    device-to-device copies inside the process."""

    def __init__(self, k, devices, min_quality=None, capacity_hint=0, trace=False, path=None):
        if not (1 <= int(k) <= 32):
            raise KmerLengthError(int(k))
        cfg = KhConfig(C.sizeof(KhConfig), int(k), -1 if min_quality is None else int(min_quality), -1,
                       int(capacity_hint), None,
                       (FLAG_TRACE if trace else 0) | {None: 0, "auto": 0, "direct": FLAG_FORCE_DIRECT,
                                                       "partition": FLAG_FORCE_PARTITION}[path], 0)
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        g = _P()
        rc = lib().kh_group_create(C.byref(g), C.byref(cfg), devs, len(devices))
        if rc != KH_OK:
            raise KmerHipError(rc)
        self._g = g
        self.counters = [DeviceCounter._adopt(lib().kh_group_ctx(g, i), k, min_quality) for i in range(len(devices))]

    def __len__(self):
        return len(self.counters)

    def __getitem__(self, i):
        return self.counters[i]

    def merge(self):
        infos = (KhMergeInfo * len(self.counters))()
        rc = lib().kh_group_merge(self._g, infos)
        if rc != KH_OK:
            detail = "; ".join(lib().kh_last_error(c._h).decode() for c in self.counters)
            raise KmerHipError(rc, detail)
        return [merge_info_dict(i) for i in infos]

    def close(self):
        if getattr(self, "_g", None):
            for c in self.counters:
                c._h = None
            lib().kh_group_destroy(self._g)
            self._g = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- host memory the device reaches directly --------------------------------
class PinnedArray:
    """A numpy view of kh_host_alloc'ed (pinned) memory: push() / push_text() from it and result(out=...) into it move
    by DMA, without the staging copies pageable memory needs.  Free with close() (or the context manager)."""

    def __init__(self, n, dtype=np.uint8):
        self.dtype = np.dtype(dtype)
        self.nbytes = int(n) * self.dtype.itemsize
        p = _P()
        rc = lib().kh_host_alloc(C.byref(p), max(self.nbytes, 1))
        if rc != KH_OK:
            raise KmerHipError(rc)
        self._p = p
        buf = (C.c_uint8 * max(self.nbytes, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(n))

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            lib().kh_host_free(self._p)
            self._p = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def host_register(arr):
    """hipHostRegister the memory of a contiguous numpy array (kh_host_register); pair with host_unregister."""
    rc = lib().kh_host_register(arr.ctypes.data, arr.nbytes)
    if rc != KH_OK:
        raise KmerHipError(rc)


def host_unregister(arr):
    rc = lib().kh_host_unregister(arr.ctypes.data)
    if rc != KH_OK:
        raise KmerHipError(rc)


# ---- pure helpers (host) ----------------------------------------------------

def pack(seq):
    if isinstance(seq, str):
        seq = seq.encode()
    out = _U64(0)
    pos = C.c_uint32(0)
    rc = lib().kh_pack(seq, len(seq), C.byref(out), C.byref(pos))
    if rc == KH_ERR_BAD_K:
        raise KmerLengthError(len(seq))
    if rc != KH_OK:
        b = seq[pos.value]  # Display of InvalidBaseError, src/error.rs:106-122
        if 0x20 <= b < 0x7F:
            raise ValueError(f"invalid base '{chr(b)}' (0x{b:02x}) at position {pos.value}")
        raise ValueError(f"invalid base 0x{b:02x} at position {pos.value}")
    return int(out.value)


def unpack(bits, k):
    if not (1 <= k <= 32):
        raise KmerLengthError(k)
    buf = C.create_string_buffer(k)
    lib().kh_unpack(int(bits), k, buf)
    return buf.raw.decode()


def canonical(bits, k):
    out = _U64(0)
    rc_flag = C.c_int(0)
    rc = lib().kh_canonical(int(bits), k, C.byref(out), C.byref(rc_flag))
    if rc == KH_ERR_BAD_K:
        raise KmerLengthError(k)
    return int(out.value), bool(rc_flag.value)


def owner(key, k, nparts):
    """Owner shard of a packed canonical k-mer (fast-range of the top bits of the table hash)."""
    return int(lib().kh_owner(int(key), int(k), int(nparts)))


def synth_reads_device(d_bases, d_qual, seed, genome_len, read_len, first_read, n_reads, device=-1, stream=None):
    rc = lib().kh_synth_reads_device(int(device), stream, int(seed), int(genome_len), int(read_len),
                                     int(first_read), int(n_reads), d_bases, d_qual)
    if rc != KH_OK:
        raise KmerHipError(rc)
