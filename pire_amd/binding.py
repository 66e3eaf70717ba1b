"""ctypes binding of libpire_hip.so (include/pire_hip.h).  No scan logic lives here."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(HERE, "libpire_hip.so")
if os.environ.get("PIRE_HIP_LIB"):   # an alternative build of the same library (tools/ab: tuning / older builds)
    _LIB_PATH = os.path.abspath(os.environ["PIRE_HIP_LIB"])

FLAG_BEGIN = 1
FLAG_END = 2
FLAG_ON_DEVICE = 4
FLAG_GENERIC = 8
FLAG_HOST_OFFSETS = 16
FLAG_NO_PEEK = 32

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)


class PireHipError(RuntimeError):
    """Counterpart of Pire::Error (pire/stub/stl.h:213-217) for the C ABI's negative return codes."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"pire_hip error {code}: {msg}")
        self.code = code


class TableInfo(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("states", C.c_uint32),
        ("letters", C.c_uint32),
        ("regexps", C.c_uint32),
        ("initial", C.c_uint32),
        ("empty", C.c_uint32),
        ("header_size", C.c_uint32),
        ("row_stride", C.c_uint32),
        ("hot_states", C.c_uint32),
        ("lds_table_bytes", C.c_uint32),
        ("device_bytes", C.c_uint64),
        ("ref_buf_size", C.c_uint64),
        ("last_trap_samples", C.c_uint64),
        ("adaptations", C.c_uint32),
        ("compact_states", C.c_uint32),
        ("scanner_type", C.c_uint32),
        ("zip_full_states", C.c_uint32),
        ("wide_states", C.c_uint32),
        ("wide_lds_bytes", C.c_uint32),
        ("outside_dense_share", C.c_float),
        ("outside_wide_share", C.c_float),
        ("shares_measured", C.c_uint32),
        ("zip_outside_share", C.c_float),
        ("last_wide_trap_chunks", C.c_uint64),
        ("wide_outside_chunk_share", C.c_float),
        ("zip_plain_outside_share", C.c_float),
    ]


class CountingInfo(C.Structure):
    _fields_ = [("states", C.c_uint32), ("letters", C.c_uint32), ("regexps", C.c_uint32), ("initial", C.c_uint32)]


class SlowInfo(C.Structure):
    _fields_ = [("states", C.c_uint32), ("letters", C.c_uint32), ("start", C.c_uint32), ("words", C.c_uint32),
                ("empty", C.c_uint32), ("reserved", C.c_uint32), ("mask_bytes", C.c_uint64)]


class SlowCaptureInfo(C.Structure):
    _fields_ = [("states", C.c_uint32), ("letters", C.c_uint32), ("start", C.c_uint32), ("entries", C.c_uint32),
                ("longest_list", C.c_uint32), ("init_len", C.c_uint32), ("init_matched", C.c_uint32), ("empty", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


def lib_path() -> str:
    return _LIB_PATH


def build(force: bool = False) -> str:
    """Compile libpire_hip.so in-tree for gfx950 with hipcc (works without a GPU)."""
    cmd = ["make", "-j8", "-C", os.path.join(HERE, "csrc")] + (["-B"] if force else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libpire_hip.so failed:\n" + r.stdout)
    return _LIB_PATH


_lib = None

class Config(C.Structure):
    """pire_hip_config (include/pire_hip.h): the library's runtime knobs, set through the ABI."""
    _fields_ = [
        ("size", C.c_uint32),
        ("tiled_variant", C.c_uint32),
        ("checked", C.c_uint32),
        ("no_compact", C.c_uint32),
        ("prior_flat", C.c_uint32),
        ("ragged_act_always", C.c_uint32),
        ("no_ragged_act", C.c_uint32),
        ("no_segments", C.c_uint32),
        ("segment_no_grid", C.c_uint32),
        ("segment_stats", C.c_uint32),
        ("segment_modes", C.c_uint32),
        ("segment_bytes", C.c_uint64),
        ("segment_warmup", C.c_uint64),
        ("segment_budget", C.c_uint64),
        ("host_chunk_bytes", C.c_uint64),
        ("host_one_shot", C.c_uint32),
        ("no_rccl", C.c_uint32),
        ("slow_sets_in_memory", C.c_uint32),
        ("slow_no_list", C.c_uint32),
        ("auto_adapt", C.c_uint32),
        ("auto_adapt_min_traps", C.c_uint32),
        ("ragged_variant", C.c_uint32),
        ("host_staging", C.c_uint32),
        ("no_offsets_peek", C.c_uint32),
        ("segment_no_pair", C.c_uint32),
        ("segment_no_product", C.c_uint32),
        ("segment_no_derive", C.c_uint32),
        ("no_length_order", C.c_uint32),
        ("capture_by_length", C.c_uint32),
        ("force_rccl", C.c_uint32),
        ("counting_variant", C.c_uint32),
        ("slow_stats", C.c_uint32),
        ("walk_variant", C.c_uint32),
        ("selftest", C.c_uint32),
        ("zip_variant", C.c_uint32),
    ]


NONE = (1 << 64) - 1   # PIRE_HIP_SEGMENT_WARMUP_NONE / PIRE_HIP_SEGMENT_BUDGET_NONE: "really zero", 0 being "the default"


ABI_VERSION = 6   # include/pire_hip.h PIRE_HIP_ABI_VERSION
SPLIT_TILE = 16384   # include/pire_hip.h PIRE_HIP_SPLIT_TILE_BYTES: the split pass cuts raw into tiles of this many bytes
GATHER_TILE = 16384   # include/pire_hip.h PIRE_HIP_GATHER_TILE_BYTES: the gather's copy pass cuts out_text into tiles of this many bytes
NO_TAIL = (1 << 32) - 1   # include/pire_hip.h PIRE_HIP_GATHER_NO_TAIL: no byte behind the gathered strings
FIELDS_TILE = 16384   # include/pire_hip.h PIRE_HIP_FIELDS_TILE_BYTES: the fields pass cuts text into tiles of this many bytes
COUNT_ALL = 1   # include/pire_hip.h PIRE_HIP_COUNT_ALL (in `mode`): every wanted regexp reaches its threshold
FINAL_SELECT_ZERO = 1   # include/pire_hip.h PIRE_HIP_FINAL_SELECT_ZERO (`mode`): the strings whose Final flag is NOT set
CONTEXT_HIT = 1   # include/pire_hip.h PIRE_HIP_CONTEXT_HIT (out_line_flags): the line is itself in the hit list
CONTEXT_GROUP = 2   # include/pire_hip.h PIRE_HIP_CONTEXT_GROUP (out_line_flags): the first line of a run of selected lines
FILES_WITHOUT = 1   # include/pire_hip.h PIRE_HIP_FILES_WITHOUT (`file_mode`): list the files with no hit (grep -L)
FIELDS_REST = 1   # include/pire_hip.h PIRE_HIP_FIELDS_REST (in `mode`): the span runs to the end of the string, `cut -f k-`
AFFIX_HEAD, AFFIX_TAIL, AFFIX_REST = 0, 1, 2   # include/pire_hip.h PIRE_HIP_AFFIX_HEAD / _TAIL / _REST (`part`)
AFFIX_LONGEST, AFFIX_THROUGH_BEGIN, AFFIX_THROUGH_END = 1, 2, 4   # include/pire_hip.h PIRE_HIP_AFFIX_* (`head_opts`, `tail_opts`)
SEARCH_SHORTEST, SEARCH_THROUGH_BEGIN, SEARCH_THROUGH_END = 1, 2, 4   # include/pire_hip.h PIRE_HIP_SEARCH_* (`opts`)
LEX_SHORTEST, LEX_THROUGH_BEGIN, LEX_THROUGH_END, LEX_TOKENS = 1, 2, 4, 8   # include/pire_hip.h PIRE_HIP_LEX_* (`opts`)
LEX_GAP = 0xFFFFFFFF   # the label of a gap (lex_labels)
SPLICE_KEEP, SPLICE_FIRST, SPLICE_PIECE_MAX = 1, 2, 256                 # include/pire_hip.h PIRE_HIP_SPLICE_* (`mode`)

# every symbol include/pire_hip.h declares: (name, restype, argtypes)
ABI = [
    ("pire_hip_build_info", C.c_char_p, []),
    ("pire_hip_config_get", C.c_int, [C.POINTER(Config)]),
    ("pire_hip_config_set", C.c_int, [C.POINTER(Config)]),
    ("pire_hip_table_create", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("pire_hip_table_mmap", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("pire_hip_table_create_from_file", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    ("pire_hip_table_glue", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("pire_hip_table_glue_gpu", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("pire_hip_table_upload", C.c_int, [C.c_void_p]),
    ("pire_hip_table_adapt", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("pire_hip_table_destroy", None, [C.c_void_p]),
    ("pire_hip_table_get_info", C.c_int, [C.c_void_p, C.POINTER(TableInfo)]),
    ("pire_hip_table_final", C.c_int, [C.c_void_p, C.c_uint32]),
    ("pire_hip_table_dead", C.c_int, [C.c_void_p, C.c_uint32]),
    ("pire_hip_table_accepted_regexps", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(u64p), C.POINTER(C.c_size_t)]),
    ("pire_hip_table_letter_class", C.c_int, [C.c_void_p, C.c_uint32]),
    ("pire_hip_table_next", C.c_int64, [C.c_void_p, C.c_uint32, C.c_uint32]),
    ("pire_hip_table_layout", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_table_wide_layout", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32)]),
    ("pire_hip_table_get_info_sized", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("pire_hip_abi_version", C.c_uint32, []),
    ("pire_hip_selftested_kernels", C.c_char_p, []),
    ("pire_hip_table_config_set", C.c_int, [C.c_void_p, C.c_void_p]),
    ("pire_hip_table_config_get", C.c_int, [C.c_void_p, C.c_void_p]),
    ("pire_hip_table_zip_layout", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    ("pire_hip_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_strided", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_step", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    ("pire_hip_table_mask_words", C.c_uint32, [C.c_void_p]),
    ("pire_hip_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_void_p]),
    ("pire_hip_run_select_strided", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_route", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_route", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_route_strided", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.c_void_p]),
    ("pire_hip_run_lines_route", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_split", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                 C.c_void_p]),
    ("pire_hip_run_lines_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                  C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_gather_spans", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_lines_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    ("pire_hip_fields", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                  C.c_void_p]),
    ("pire_hip_run_lines_field_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                  C.c_void_p, C.c_void_p]),
    ("pire_hip_run_lines_field_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                                  C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_half_final", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_prefix", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                  C.c_void_p, C.c_void_p]),
    ("pire_hip_suffix", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                  C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_table_create", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("pire_hip_slow_table_destroy", None, [C.c_void_p]),
    ("pire_hip_slow_table_get_info", C.c_int, [C.c_void_p, C.POINTER(SlowInfo)]),
    ("pire_hip_slow_table_plan", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32 * 24)]),
    ("pire_hip_slow_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_run_strided", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_counting_table_create", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("pire_hip_counting_table_destroy", None, [C.c_void_p]),
    ("pire_hip_counting_table_get_info", C.c_int, [C.c_void_p, C.POINTER(CountingInfo)]),
    ("pire_hip_counting_table_forms", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32 * 8)]),
    ("pire_hip_counting_run", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    ("pire_hip_capture_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_capture_select", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_capture_run_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                              C.c_void_p]),
    ("pire_hip_capture_lines_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_count_select", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_counting_run_select", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_half_final_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_counting_lines_select", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_half_final_lines_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_final_select", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_run_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_run_select_strided", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_lines_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_lines_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_capture_table_create", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("pire_hip_slow_capture_table_destroy", None, [C.c_void_p]),
    ("pire_hip_slow_capture_table_get_info", C.c_int, [C.c_void_p, C.POINTER(SlowCaptureInfo)]),
    ("pire_hip_slow_capture_table_image", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_capture_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_capture_run_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_capture_lines_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_affix_select", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_affix_run_select", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_affix_lines_gather", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_search", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_search_run_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_search_lines_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_search_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_search_all_lines_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_lex", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_lex_lines_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_splice", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_search_lines_splice", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_context", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_lines_context_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_lines_context_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_lines_context_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_lines_context_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_files", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_lines_files_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_slow_lines_files_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_combine", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("pire_hip_lines_combine_select", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_lines_combine_gather", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_multi_create", C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    ("pire_hip_multi_destroy", None, [C.c_void_p]),
    ("pire_hip_multi_device_count", C.c_int, [C.c_void_p]),
    ("pire_hip_multi_reduce_backend", C.c_char_p, [C.c_void_p]),
    ("pire_hip_multi_run_strided", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("pire_hip_multi_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("pire_hip_multi_run_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_multi_last_split", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    ("pire_hip_multi_run_strided_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_last_kernel", C.c_char_p, []),
    ("pire_hip_last_kernel_symbol", C.c_char_p, []),
    ("pire_hip_set_timing", C.c_int, [C.c_int]),
    ("pire_hip_last_kernel_ms", C.c_float, []),
    ("pire_hip_last_error", C.c_char_p, []),
    ("pire_hip_device_count", C.c_int, []),
    ("pire_hip_run_pair", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_run_pair_strided", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pire_hip_table_check_failures", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("pire_hip_host_alloc", C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    ("pire_hip_host_free", None, [C.c_void_p]),
    ("pire_hip_device_alloc", C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    ("pire_hip_device_free", None, [C.c_void_p]),
    ("pire_hip_copy_to_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("pire_hip_copy_to_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("pire_hip_memset_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    ("pire_hip_stream_synchronize", C.c_int, [C.c_void_p]),
    ("pire_hip_corpus_fill", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                       C.c_void_p, C.c_void_p]),
]


def lib():
    """Load the native library.  Fails loudly if it has not been built: there is no Python/CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C pire_amd/csrc` (hipcc, gfx950). pire_amd has no CPU fallback.")
        # PyTorch-ROCm bundles its own libamdhip64.so.7; a process must hold exactly ONE HIP runtime or the second
        # one finds no devices.  Let torch's copy load first so that our NEEDED libamdhip64.so.7 binds to it.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_LIB_PATH)
        for name, res, args in ABI:
            try:
                fn = getattr(L, name)
            except AttributeError:
                if os.environ.get("PIRE_HIP_LIB"):   # an older build under tools/ab: entry points added since are absent
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        # the structs declared above are THIS header's (include/pire_hip.h PIRE_HIP_ABI_VERSION): a library of another version
        # would write a pire_hip_table_info of another size into them
        if not os.environ.get("PIRE_HIP_LIB") and hasattr(L, "pire_hip_abi_version") and L.pire_hip_abi_version() != ABI_VERSION:
            raise ImportError(f"{_LIB_PATH} is ABI version {L.pire_hip_abi_version()}, this binding is {ABI_VERSION}: rebuild")
        _lib = L
    return _lib


def get_config() -> Config:
    c = Config()
    c.size = C.sizeof(Config)
    _check(lib().pire_hip_config_get(C.byref(c)))
    return c


def set_config(**fields) -> Config:
    """Change the named pire_hip_config fields (process-wide); returns the configuration as it was before."""
    old = get_config()
    new = get_config()
    for k, v in fields.items():
        if k not in dict(Config._fields_) or k == "size":
            raise KeyError(k)
        setattr(new, k, int(v))
    _check(lib().pire_hip_config_set(C.byref(new)))
    return old


class config:
    """`with config(tiled_variant=22): ...` -- the fields changed inside the block, restored after it."""

    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self):
        self.old = set_config(**self.fields)
        return self

    def __exit__(self, *exc):
        _check(lib().pire_hip_config_set(C.byref(self.old)))
        return False


def device_count() -> int:
    return lib().pire_hip_device_count()


def _check(rc: int):
    if rc < 0:
        raise PireHipError(rc, lib().pire_hip_last_error().decode(errors="replace"))
    return rc


def _np_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


# --- raw text into strings (pire_hip_split)
def _raw_bytes(raw) -> np.ndarray:
    return np.ascontiguousarray(np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else raw, dtype=np.uint8)


def split_host(raw, delim: int = 10, keep_delim: bool = False, offsets_cap: Optional[int] = None):
    """pire_hip_split on host arrays: (text u8 -- None with keep_delim --, offsets u64[min(n, cap) + 1], n).  offsets_cap
    None = room for every string: one call for n, one for the rest."""
    raw = _raw_bytes(raw)
    n = C.c_uint64(0)
    ptr = raw.ctypes.data if raw.size else None
    if offsets_cap is None:
        _check(lib().pire_hip_split(ptr, raw.size, delim, 0, None, None, 0, C.byref(n), None))
        offsets_cap = int(n.value)
    text = None if keep_delim else np.zeros(max(raw.size, 1), dtype=np.uint8)
    offsets = np.zeros(offsets_cap + 1, dtype=np.uint64)
    _check(lib().pire_hip_split(ptr, raw.size, delim, 0, _np_ptr(text), offsets.ctypes.data, offsets_cap, C.byref(n), None))
    k = min(int(n.value), offsets_cap)
    delims = int(n.value) - (1 if raw.size and int(raw[-1]) != delim else 0)
    return (None if text is None else text[:raw.size - delims]), offsets[:k + 1], int(n.value)


def split_device(raw_ptr: int, size: int, out_n_ptr: int, delim: int = 10, out_text_ptr=0, out_offsets_ptr=0, offsets_cap=0,
                 stream: int = 0):
    """pire_hip_split with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_split(raw_ptr or None, size, delim, FLAG_ON_DEVICE, out_text_ptr or None, out_offsets_ptr or None,
                                offsets_cap, out_n_ptr or None, stream or None))


# --- the listed strings of a batch back to back (pire_hip_gather / pire_hip_gather_spans)
def _tail(tail) -> int:
    return NO_TAIL if tail is None else int(tail)


def gather_host(text, offsets=None, idx=None, tail=None, spans=None, text_cap: Optional[int] = None):
    """pire_hip_gather on host arrays -- or, with spans (uint64[k, 2], begin / end in `text`), pire_hip_gather_spans:
    (out_text u8[min(total, text_cap)], out_offsets u64[k + 1], total).  tail None = no byte behind the strings; text_cap
    None = room for everything (the sources' lengths are the host's to add up)."""
    text = _raw_bytes(text)
    a = 0 if tail is None else 1
    if spans is not None:
        spans = np.ascontiguousarray(spans, dtype=np.uint64).reshape(-1, 2)
        k = len(spans)
        room = int((spans[:, 1] - spans[:, 0]).sum()) + a * k if text_cap is None else int(text_cap)
    else:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint64)
        k = len(offsets) - 1 if idx is None else len(idx)
        src = np.arange(k, dtype=np.int64) if idx is None else idx.astype(np.int64)
        room = int((offsets[src + 1] - offsets[src]).sum()) + a * k if text_cap is None else int(text_cap)
    out = np.zeros(max(room, 1), dtype=np.uint8)
    out_offsets = np.zeros(k + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    tptr = text.ctypes.data if text.size else None
    if spans is not None:
        _check(lib().pire_hip_gather_spans(tptr, text.size, spans.ctypes.data if k else None, None, k, _tail(tail), 0,
                                           out.ctypes.data if room else None, room, out_offsets.ctypes.data, C.byref(total), None))
    else:
        _check(lib().pire_hip_gather(tptr, offsets.ctypes.data, len(offsets) - 1, _np_ptr(idx) if k else None, None, k, _tail(tail), 0,
                                     out.ctypes.data if room else None, room, out_offsets.ctypes.data, C.byref(total), None))
    return out[:min(int(total.value), room)], out_offsets, int(total.value)


def gather_device(text_ptr: int, offsets_ptr: int, n: int, out_bytes_ptr: int, idx_ptr=0, idx_count_ptr=0, idx_cap=0, tail=None,
                  out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
    """pire_hip_gather with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_gather(text_ptr or None, offsets_ptr or None, n, idx_ptr or None, idx_count_ptr or None, idx_cap, _tail(tail),
                                 FLAG_ON_DEVICE, out_text_ptr or None, text_cap, out_offsets_ptr or None, out_bytes_ptr or None,
                                 stream or None))


def gather_spans_device(raw_ptr: int, size: int, spans_ptr: int, out_bytes_ptr: int, span_count_ptr=0, span_cap=0, tail=None,
                        out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
    """pire_hip_gather_spans with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_gather_spans(raw_ptr or None, size, spans_ptr or None, span_count_ptr or None, span_cap, _tail(tail),
                                       FLAG_ON_DEVICE, out_text_ptr or None, text_cap, out_offsets_ptr or None, out_bytes_ptr or None,
                                       stream or None))


# --- one column of every string (pire_hip_fields)
def fields_host(text, offsets, field: int, sep: int = 9, rest: bool = False):
    """pire_hip_fields on host arrays: spans uint64[n, 2], begin / end of field `field` (from 0) of every string in `text`."""
    text = _raw_bytes(text)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    spans = np.zeros((n, 2), dtype=np.uint64)
    _check(lib().pire_hip_fields(text.ctypes.data if text.size else None, offsets.ctypes.data, n, sep, field,
                                 FIELDS_REST if rest else 0, 0, spans.ctypes.data if n else None, None))
    return spans


def fields_device(text_ptr: int, offsets_ptr: int, n: int, field: int, out_spans_ptr: int, sep: int = 9, rest: bool = False,
                  stream: int = 0):
    """pire_hip_fields with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_fields(text_ptr or None, offsets_ptr or None, n, sep, field, FIELDS_REST if rest else 0, FLAG_ON_DEVICE,
                                 out_spans_ptr or None, stream or None))


# --- from result rows to the strings that count (pire_hip_count_select)
def _min_count(min_count, regexps):
    if min_count is None:
        return None
    m = np.ascontiguousarray(min_count, dtype=np.uint32)
    if m.shape != (regexps,):
        raise ValueError("min_count needs one entry per regexp")
    return m


class _CountOut:
    """The host arrays of one count-select call and what comes back in them."""

    def __init__(self, regexps, room, hit_cap, totals, hits, hit_results):
        self.regexps = regexps
        self.cap = room if hit_cap is None else int(hit_cap)
        self.totals = np.zeros(regexps, dtype=np.uint64) if totals else None
        self.hits = np.zeros(self.cap, dtype=np.uint64) if hits else None
        self.rows = np.zeros((self.cap, regexps), dtype=np.uint32) if hit_results else None
        self.cnt = C.c_uint64(0)

    def args(self):
        lists = self.cap > 0
        return (_np_ptr(self.totals) if self.regexps else None, _np_ptr(self.hits) if lists else None,
                _np_ptr(self.rows) if lists and self.regexps else None, self.cap, C.byref(self.cnt))

    def result(self):
        count = int(self.cnt.value)
        k = min(count, self.cap)
        return {"totals": self.totals, "hits": None if self.hits is None else self.hits[:k],
                "hit_results": None if self.rows is None else self.rows[:k], "count": count}


def count_select_host(results, min_count=None, all=False, hit_cap: Optional[int] = None, totals=True, hits=True, hit_results=True):
    """pire_hip_count_select on a host array results[n, regexps]: {"totals" u64[R], "hits" u64[k], "hit_results" u32[k, R],
    "count"}, k = min(count, hit_cap); what was not asked for is None.  hit_cap None = room for every string."""
    results = np.ascontiguousarray(results, dtype=np.uint32)
    n, regexps = results.shape
    m = _min_count(min_count, regexps)
    out = _CountOut(regexps, n, hit_cap, totals, hits, hit_results)
    _check(lib().pire_hip_count_select(results.ctypes.data if results.size else None, n, regexps, _np_ptr(m), COUNT_ALL if all else 0, 0,
                                       *out.args(), None))
    return out.result()


def count_select_device(results_ptr: int, n: int, regexps: int, out_hit_count_ptr: int, min_count_ptr=0, all=False, out_totals_ptr=0,
                        out_hits_ptr=0, out_hit_results_ptr=0, hit_cap=0, stream: int = 0):
    """pire_hip_count_select with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_count_select(results_ptr or None, n, regexps, min_count_ptr or None, COUNT_ALL if all else 0, FLAG_ON_DEVICE,
                                       out_totals_ptr or None, out_hits_ptr or None, out_hit_results_ptr or None, hit_cap,
                                       out_hit_count_ptr or None, stream or None))


# --- from capture positions to byte ranges (pire_hip_capture_select)
# --- from Final flags to the strings that matched, or did not (pire_hip_final_select)
def _final_mode(invert) -> int:
    return FINAL_SELECT_ZERO if invert else 0


def final_select_host(final, invert=False, hit_cap: Optional[int] = None):
    """pire_hip_final_select on a host array final[n]: {"hits" u64[k], "count"}, k = min(count, hit_cap); hit_cap None = room
    for every string."""
    final = np.ascontiguousarray(final, dtype=np.uint8)
    n = final.size
    cap = n if hit_cap is None else int(hit_cap)
    hits = np.zeros(cap, dtype=np.uint64)
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_final_select(final.ctypes.data if n else None, n, _final_mode(invert), 0, hits.ctypes.data if cap else None, cap,
                                       C.byref(cnt), None))
    return {"hits": hits[:min(int(cnt.value), cap)], "count": int(cnt.value)}


def final_select_device(final_ptr: int, n: int, out_hit_count_ptr: int, invert=False, out_hits_ptr=0, hit_cap=0, stream: int = 0):
    """pire_hip_final_select with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_final_select(final_ptr or None, n, _final_mode(invert), FLAG_ON_DEVICE, out_hits_ptr or None, hit_cap,
                                       out_hit_count_ptr or None, stream or None))


# --- from a hit list to the hits and their neighbours (pire_hip_context and the lines forms on top of it)
def context_host(hits, n: int, before: int = 0, after: int = 0, hit_count: Optional[int] = None, line_cap: Optional[int] = None,
                 want_lines=True, want_flags=True, want_groups=True):
    """pire_hip_context on a host list hits[k]: {"lines" u64[m] or None, "flags" u8[m] or None, "count", "groups" or None},
    m = min(count, line_cap); line_cap None = room for every line; hit_count None = no hit_count pointer (k = hits.size)."""
    hits = np.ascontiguousarray(hits, dtype=np.uint64)
    cap = int(n) if line_cap is None else int(line_cap)
    lines = np.zeros(cap, dtype=np.uint64) if want_lines else None
    flags = np.zeros(cap, dtype=np.uint8) if want_flags else None
    k = None if hit_count is None else C.c_uint64(int(hit_count))
    cnt, groups = C.c_uint64(0), C.c_uint64(0)
    _check(lib().pire_hip_context(hits.ctypes.data if hits.size else None, None if k is None else C.byref(k), hits.size, n, before, after, 0,
                                  lines.ctypes.data if want_lines and cap else None, flags.ctypes.data if want_flags and cap else None,
                                  cap, C.byref(cnt), C.byref(groups) if want_groups else None, None))
    m = min(int(cnt.value), cap)
    return {"lines": lines[:m] if want_lines else None, "flags": flags[:m] if want_flags else None, "count": int(cnt.value),
            "groups": int(groups.value) if want_groups else None}


def context_device(hits_ptr: int, hit_cap: int, n: int, out_line_count_ptr: int, before: int = 0, after: int = 0, hit_count_ptr=0,
                   out_lines_ptr=0, out_line_flags_ptr=0, line_cap=0, out_group_count_ptr=0, stream: int = 0):
    """pire_hip_context with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_context(hits_ptr or None, hit_count_ptr or None, hit_cap, n, before, after, FLAG_ON_DEVICE, out_lines_ptr or None,
                                  out_line_flags_ptr or None, line_cap, out_line_count_ptr or None, out_group_count_ptr or None,
                                  stream or None))


def _lines_context_host(select, gather, front, raw, delim, before, after, tail, line_cap, text_cap, with_text):
    """the host form of the four lines forms: front = the arguments between flags and before (want / mode)"""
    raw = _raw_bytes(raw)
    cap = raw.size if line_cap is None else int(line_cap)
    lines = np.zeros(cap, dtype=np.uint64)
    flags = np.zeros(cap, dtype=np.uint8)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    n, sel, groups, hit = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    args = front + [before, after, C.byref(n), lines.ctypes.data if cap else None, flags.ctypes.data if cap else None,
                    spans.ctypes.data if cap else None, cap, C.byref(sel), C.byref(groups), C.byref(hit)]
    if not with_text:
        _check(select(*args, None))
    else:
        room = raw.size + cap if text_cap is None else int(text_cap)
        text = np.zeros(max(room, 1), dtype=np.uint8)
        offsets = np.zeros(cap + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        _check(gather(*args, _tail(delim if tail == -1 else tail), text.ctypes.data if room else None, room, offsets.ctypes.data,
                      C.byref(total), None))
    k = min(int(sel.value), cap)
    out = {"lines": int(n.value), "context": lines[:k], "flags": flags[:k], "spans": spans[:k], "count": int(sel.value),
           "groups": int(groups.value), "hits": int(hit.value)}
    if with_text:
        out.update({"text": text[:min(int(total.value), room)], "offsets": offsets[:k + 1], "bytes": int(total.value)})
    return out


def _lines_context_device(select, gather, front, before, after, delim, tail, out_line_count_ptr, out_sel_count_ptr, out_lines_ptr,
                          out_line_flags_ptr, out_line_spans_ptr, line_cap, out_group_count_ptr, out_hit_count_ptr, out_bytes_ptr,
                          out_text_ptr, text_cap, out_offsets_ptr, stream):
    args = front + [before, after, out_line_count_ptr or None, out_lines_ptr or None, out_line_flags_ptr or None,
                    out_line_spans_ptr or None, line_cap, out_sel_count_ptr or None, out_group_count_ptr or None,
                    out_hit_count_ptr or None]
    if out_bytes_ptr is None:
        _check(select(*args, stream or None))
    else:
        _check(gather(*args, _tail(delim if tail == -1 else tail), out_text_ptr or None, text_cap, out_offsets_ptr or None,
                      out_bytes_ptr or None, stream or None))


# --- boolean queries over hit lists (pire_hip_combine and the lines forms on top of it)
COMBINE_MAX_LISTS = 6   # include/pire_hip.h PIRE_HIP_COMBINE_MAX_LISTS
TERM_LINE = 0xFFFFFFFF   # include/pire_hip.h PIRE_HIP_TERM_LINE (`column`): the term scans the whole line


def truth(k: int, fn) -> int:
    """The truth table of pire_hip_combine over k lists from a Python predicate over the member mask: bit m is set where
    fn(m) holds, m = sum of 1 << j over the lists j a line is in.  truth(2, lambda m: m == 1): in list 0 and not in list 1."""
    if not 1 <= int(k) <= COMBINE_MAX_LISTS:
        raise ValueError(f"truth: k = {k}, 1 .. {COMBINE_MAX_LISTS} lists")
    return sum(1 << m for m in range(1 << int(k)) if fn(m))


def _combine_arrays(ptrs, count_ptrs, caps):
    """the three host arrays of pire_hip_combine (count_ptrs None: a null list_counts)"""
    k = len(ptrs)
    lists = (C.c_void_p * max(k, 1))(*[p or None for p in ptrs])
    counts = None if count_ptrs is None else (C.c_void_p * max(k, 1))(*[p or None for p in count_ptrs])
    return lists, counts, (C.c_uint64 * max(k, 1))(*[int(c) for c in caps])


def combine_host(lists, n: int, truth_bits: int, list_counts=None, hit_cap: Optional[int] = None, want_hits=True, want_members=True):
    """pire_hip_combine on host lists (a sequence of uint64 arrays): {"hits" u64[m] or None, "members" u8[m] or None, "count"},
    m = min(count, hit_cap); hit_cap None = room for every line; list_counts None = no list_counts array, else one entry per
    list (an int, or None for a null pointer)."""
    arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in lists]
    cap = int(n) if hit_cap is None else int(hit_cap)
    hits = np.zeros(cap, dtype=np.uint64) if want_hits else None
    members = np.zeros(cap, dtype=np.uint8) if want_members else None
    ks = None if list_counts is None else [None if c is None else C.c_uint64(int(c)) for c in list_counts]
    pl, pc, caps = _combine_arrays([a.ctypes.data if a.size else 0 for a in arrs],
                                   None if ks is None else [0 if c is None else C.addressof(c) for c in ks], [a.size for a in arrs])
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_combine(pl, pc, caps, len(arrs), n, truth_bits, 0, hits.ctypes.data if want_hits and cap else None,
                                  members.ctypes.data if want_members and cap else None, cap, C.byref(cnt), None))
    m = min(int(cnt.value), cap)
    return {"hits": hits[:m] if want_hits else None, "members": members[:m] if want_members else None, "count": int(cnt.value)}


def combine_device(list_ptrs, list_caps, n: int, truth_bits: int, out_hit_count_ptr: int, list_count_ptrs=None, out_hits_ptr=0,
                   out_hit_members_ptr=0, hit_cap=0, stream: int = 0):
    """pire_hip_combine with PIRE_HIP_RUN_ON_DEVICE: raw device addresses (the sequences themselves are the host's), only
    enqueues on `stream`."""
    pl, pc, caps = _combine_arrays(list_ptrs, list_count_ptrs, list_caps)
    _check(lib().pire_hip_combine(pl, pc, caps, len(list_ptrs), n, truth_bits, FLAG_ON_DEVICE, out_hits_ptr or None,
                                  out_hit_members_ptr or None, hit_cap, out_hit_count_ptr or None, stream or None))


class LineTerm(C.Structure):
    """pire_hip_line_term (include/pire_hip.h)."""
    _fields_ = [("table", C.c_void_p), ("slow_table", C.c_void_p), ("want", C.c_void_p), ("mode", C.c_uint32),
                ("run_flags", C.c_uint32), ("column", C.c_uint32), ("sep", C.c_uint32), ("field_mode", C.c_uint32)]


def line_term(table=None, slow_table=None, want_ptr=0, invert=False, flags=FLAG_BEGIN | FLAG_END, column: Optional[int] = None,
              sep: int = 9, rest=False) -> LineTerm:
    """One term of the lines forms: a Table (want_ptr: `want`, on the side the call's other pointers live) or a SlowTable
    (invert: the lines it does not match), on the whole line (column None) or on one column."""
    t = LineTerm()
    t.table = None if table is None else table._h
    t.slow_table = None if slow_table is None else slow_table._h
    t.want = want_ptr or None
    t.mode = _final_mode(invert)
    t.run_flags = flags
    t.column = TERM_LINE if column is None else int(column)
    t.sep = sep
    t.field_mode = FIELDS_REST if rest else 0
    return t


def _line_terms(terms):
    return (LineTerm * max(len(terms), 1))(*terms)


def lines_combine_host(terms, truth_bits: int, raw, delim: int = 10, hit_cap: Optional[int] = None, gather=False, tail=-1,
                       text_cap: Optional[int] = None):
    """pire_hip_lines_combine_select (gather=True: _gather) on a host buffer: {"lines", "hits" u64[k], "spans" u64[k, 2],
    "members" u8[k], "count", "term_counts" u64[len(terms)]} and, gathered, "text", "offsets", "bytes"; k = min(count, hit_cap);
    tail -1 = the delimiter.  A term's want_ptr is then a host address (keep the array alive)."""
    raw = _raw_bytes(raw)
    cap = raw.size if hit_cap is None else int(hit_cap)
    hits = np.zeros(cap, dtype=np.uint64)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    members = np.zeros(cap, dtype=np.uint8)
    term_counts = np.zeros(max(len(terms), 1), dtype=np.uint64)
    n, cnt = C.c_uint64(0), C.c_uint64(0)
    args = [_line_terms(terms), len(terms), truth_bits, raw.ctypes.data if raw.size else None, raw.size, delim, 0, C.byref(n),
            hits.ctypes.data if cap else None, spans.ctypes.data if cap else None, members.ctypes.data if cap else None, cap,
            C.byref(cnt), term_counts.ctypes.data]
    if not gather:
        _check(lib().pire_hip_lines_combine_select(*args, None))
    else:
        room = raw.size + cap if text_cap is None else int(text_cap)
        text = np.zeros(max(room, 1), dtype=np.uint8)
        offsets = np.zeros(cap + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        _check(lib().pire_hip_lines_combine_gather(*args, _tail(delim if tail == -1 else tail), text.ctypes.data if room else None, room,
                                                   offsets.ctypes.data, C.byref(total), None))
    k = min(int(cnt.value), cap)
    out = {"lines": int(n.value), "hits": hits[:k], "spans": spans[:k], "members": members[:k], "count": int(cnt.value),
           "term_counts": term_counts[:len(terms)]}
    if gather:
        out.update({"text": text[:min(int(total.value), room)], "offsets": offsets[:k + 1], "bytes": int(total.value)})
    return out


def lines_combine_device(terms, truth_bits: int, raw_ptr: int, size: int, out_line_count_ptr: int, out_hit_count_ptr: int, delim: int = 10,
                         out_hits_ptr=0, out_hit_spans_ptr=0, out_hit_members_ptr=0, hit_cap=0, out_term_counts_ptr=0, tail=-1,
                         out_bytes_ptr=None, out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
    """pire_hip_lines_combine_select on device pointers -- out_bytes_ptr not None: _gather -- (synchronises `stream` once, to
    read the line count back).  A term's want_ptr is a device address."""
    args = [_line_terms(terms), len(terms), truth_bits, raw_ptr or None, size, delim, FLAG_ON_DEVICE, out_line_count_ptr or None,
            out_hits_ptr or None, out_hit_spans_ptr or None, out_hit_members_ptr or None, hit_cap, out_hit_count_ptr or None,
            out_term_counts_ptr or None]
    if out_bytes_ptr is None:
        _check(lib().pire_hip_lines_combine_select(*args, stream or None))
    else:
        _check(lib().pire_hip_lines_combine_gather(*args, _tail(delim if tail == -1 else tail), out_text_ptr or None, text_cap,
                                                   out_offsets_ptr or None, out_bytes_ptr or None, stream or None))


# --- from a hit list and file boundaries to hits by file (pire_hip_files and the lines forms on top of it)
def _file_mode(without) -> int:
    return FILES_WITHOUT if without else 0


def files_host(hits, n: int, bounds, without=False, hit_count: Optional[int] = None, file_cap: Optional[int] = None, want_first=True,
               want_hit_file=True, want_hit_line=True):
    """pire_hip_files on a host list hits[k] and bounds[files + 1]: {"first" u64[files + 1] or None, "hit_file" / "hit_line"
    u64[k] or None, "files" u64[m], "count"}, m = min(count, file_cap); file_cap None = room for every file; hit_count None =
    no hit_count pointer (k = hits.size)."""
    hits = np.ascontiguousarray(hits, dtype=np.uint64)
    bounds = np.ascontiguousarray(bounds, dtype=np.uint64)
    files = max(bounds.size - 1, 0)
    cap = files if file_cap is None else int(file_cap)
    k = None if hit_count is None else C.c_uint64(int(hit_count))
    kk = hits.size if hit_count is None else min(int(hit_count), hits.size)
    first = np.zeros(files + 1, dtype=np.uint64) if want_first else None
    hit_file = np.zeros(hits.size, dtype=np.uint64) if want_hit_file else None
    hit_line = np.zeros(hits.size, dtype=np.uint64) if want_hit_line else None
    listed = np.zeros(cap, dtype=np.uint64)
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_files(hits.ctypes.data if hits.size else None, None if k is None else C.byref(k), hits.size, n,
                                bounds.ctypes.data if bounds.size else None, files, _file_mode(without), 0, _np_ptr(first),
                                hit_file.ctypes.data if want_hit_file and hits.size else None,
                                hit_line.ctypes.data if want_hit_line and hits.size else None, listed.ctypes.data if cap else None, cap,
                                C.byref(cnt), None))
    return {"first": first, "hit_file": hit_file[:kk] if want_hit_file else None, "hit_line": hit_line[:kk] if want_hit_line else None,
            "files": listed[:min(int(cnt.value), cap)], "count": int(cnt.value)}


def files_device(hits_ptr: int, hit_cap: int, n: int, bounds_ptr: int, files: int, out_file_count_ptr: int, without=False, hit_count_ptr=0,
                 out_file_first_ptr=0, out_hit_file_ptr=0, out_hit_line_ptr=0, out_files_ptr=0, file_cap=0, stream: int = 0):
    """pire_hip_files with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_files(hits_ptr or None, hit_count_ptr or None, hit_cap, n, bounds_ptr or None, files, _file_mode(without),
                                FLAG_ON_DEVICE, out_file_first_ptr or None, out_hit_file_ptr or None, out_hit_line_ptr or None,
                                out_files_ptr or None, file_cap, out_file_count_ptr or None, stream or None))


def _lines_files_host(call, front, raw, file_bytes, without, hit_cap, file_cap):
    """the host form of the two lines forms: front = the arguments in front of file_bytes (table .. want / mode)"""
    file_bytes = np.ascontiguousarray(file_bytes, dtype=np.uint64)
    files = max(file_bytes.size - 1, 0)
    cap = raw.size if hit_cap is None else int(hit_cap)
    fcap = files if file_cap is None else int(file_cap)
    hits, hit_file, hit_line = (np.zeros(cap, dtype=np.uint64) for _ in range(3))
    spans = np.zeros((cap, 2), dtype=np.uint64)
    file_lines, first = np.zeros(files + 1, dtype=np.uint64), np.zeros(files + 1, dtype=np.uint64)
    listed = np.zeros(fcap, dtype=np.uint64)
    n, cnt, fcnt, straddles = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(call(*front, file_bytes.ctypes.data if file_bytes.size else None, files, _file_mode(without), C.byref(n),
                hits.ctypes.data if cap else None, spans.ctypes.data if cap else None, hit_file.ctypes.data if cap else None,
                hit_line.ctypes.data if cap else None, cap, C.byref(cnt), file_lines.ctypes.data, first.ctypes.data,
                listed.ctypes.data if fcap else None, fcap, C.byref(fcnt), C.byref(straddles), None))
    k = min(int(cnt.value), cap)
    return {"lines": int(n.value), "hits": hits[:k], "spans": spans[:k], "hit_file": hit_file[:k], "hit_line": hit_line[:k],
            "count": int(cnt.value), "file_lines": file_lines, "first": first, "files": listed[:min(int(fcnt.value), fcap)],
            "file_count": int(fcnt.value), "straddles": int(straddles.value)}


def _lines_files_device(call, front, file_bytes_ptr, files, without, out_line_count_ptr, out_hits_ptr, out_hit_spans_ptr, out_hit_file_ptr,
                        out_hit_line_ptr, hit_cap, out_hit_count_ptr, out_file_lines_ptr, out_file_first_ptr, out_files_ptr, file_cap,
                        out_file_count_ptr, out_straddles_ptr, stream):
    _check(call(*front, file_bytes_ptr or None, files, _file_mode(without), out_line_count_ptr or None, out_hits_ptr or None,
                out_hit_spans_ptr or None, out_hit_file_ptr or None, out_hit_line_ptr or None, hit_cap, out_hit_count_ptr or None,
                out_file_lines_ptr or None, out_file_first_ptr or None, out_files_ptr or None, file_cap, out_file_count_ptr or None,
                out_straddles_ptr or None, stream or None))


# --- from prefix and suffix lengths to matched heads and tails (pire_hip_affix_select and the forms on top of it)
def affix_opts(longest=True, through_begin=False, through_end=False) -> int:
    """the PIRE_HIP_AFFIX_* bits of one scan"""
    return (AFFIX_LONGEST if longest else 0) | (AFFIX_THROUGH_BEGIN if through_begin else 0) | (AFFIX_THROUGH_END if through_end else 0)


def _table_ptr(t):
    return None if t is None else t._h


def affix_select_host(offsets, head_len=None, tail_len=None, part=AFFIX_HEAD, hit_cap: Optional[int] = None, want_hits=True,
                      want_spans=True):
    """pire_hip_affix_select on host arrays: {"hits" u64[k] or None, "spans" u64[k, 2] or None, "count"}, k = min(count,
    hit_cap); hit_cap None = room for every string."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    head_len = None if head_len is None else np.ascontiguousarray(head_len, dtype=np.int64)
    tail_len = None if tail_len is None else np.ascontiguousarray(tail_len, dtype=np.int64)
    n = len(offsets) - 1
    cap = n if hit_cap is None else int(hit_cap)
    hits = np.zeros(cap, dtype=np.uint64) if want_hits else None
    spans = np.zeros((cap, 2), dtype=np.uint64) if want_spans else None
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_affix_select(offsets.ctypes.data, n, part, 0, _np_ptr(head_len), _np_ptr(tail_len),
                                       _np_ptr(hits) if cap else None, _np_ptr(spans) if cap else None, cap, C.byref(cnt), None))
    k = min(int(cnt.value), cap)
    return {"hits": None if hits is None else hits[:k], "spans": None if spans is None else spans[:k], "count": int(cnt.value)}


def affix_select_device(offsets_ptr: int, n: int, out_hit_count_ptr: int, head_len_ptr=0, tail_len_ptr=0, part=AFFIX_HEAD,
                        out_hits_ptr=0, out_spans_ptr=0, hit_cap=0, stream: int = 0):
    """pire_hip_affix_select with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_affix_select(offsets_ptr or None, n, part, FLAG_ON_DEVICE, head_len_ptr or None, tail_len_ptr or None,
                                       out_hits_ptr or None, out_spans_ptr or None, hit_cap, out_hit_count_ptr or None, stream or None))


def affix_run_select(head, tail, text, offsets, part=AFFIX_HEAD, head_opts=AFFIX_LONGEST, tail_opts=AFFIX_LONGEST,
                     hit_cap: Optional[int] = None, lengths=True, generic=False):
    """pire_hip_affix_run_select on host strings; head, tail: Table or None.  {"hits", "spans", "count"} and, with lengths,
    {"head_len", "tail_len"} (None for the table that is not given); without, the library keeps those arrays to itself."""
    text = _raw_bytes(text)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    cap = n if hit_cap is None else int(hit_cap)
    hl = np.empty(n, dtype=np.int64) if lengths and head is not None else None
    tl = np.empty(n, dtype=np.int64) if lengths and tail is not None else None
    hits = np.zeros(cap, dtype=np.uint64)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_affix_run_select(_table_ptr(head), head_opts, _table_ptr(tail), tail_opts, text.ctypes.data if text.size else None,
                                           offsets.ctypes.data, n, part, FLAG_GENERIC if generic else 0, _np_ptr(hl), _np_ptr(tl),
                                           hits.ctypes.data if cap else None, spans.ctypes.data if cap else None, cap, C.byref(cnt), None))
    k = min(int(cnt.value), cap)
    out = {"hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}
    if lengths:
        out.update(head_len=hl, tail_len=tl)
    return out


def affix_run_select_device(head, tail, text_ptr: int, offsets_ptr: int, n: int, out_hit_count_ptr: int, part=AFFIX_HEAD,
                            head_opts=AFFIX_LONGEST, tail_opts=AFFIX_LONGEST, out_head_len_ptr=0, out_tail_len_ptr=0, out_hits_ptr=0,
                            out_spans_ptr=0, hit_cap=0, stream: int = 0, generic=False):
    """pire_hip_affix_run_select on device pointers: only enqueues on `stream`."""
    _check(lib().pire_hip_affix_run_select(_table_ptr(head), head_opts, _table_ptr(tail), tail_opts, text_ptr or None, offsets_ptr or None, n,
                                           part, FLAG_ON_DEVICE | (FLAG_GENERIC if generic else 0), out_head_len_ptr or None,
                                           out_tail_len_ptr or None, out_hits_ptr or None, out_spans_ptr or None, hit_cap,
                                           out_hit_count_ptr or None, stream or None))


def affix_lines_gather_host(head, tail, raw, part=AFFIX_HEAD, delim: int = 10, head_opts=AFFIX_LONGEST, tail_opts=AFFIX_LONGEST,
                            tail_byte=-1, hit_cap=None, text_cap=None, gather=True):
    """pire_hip_affix_lines_gather on a host buffer: {"lines", "hits", "spans", "count"} and, with gather, {"text", "offsets",
    "bytes"}.  tail_byte -1 = the delimiter, None = none; hit_cap None = room for a hit on every line, text_cap None = for all
    of them."""
    raw = _raw_bytes(raw)
    cap = raw.size if hit_cap is None else int(hit_cap)
    room = (raw.size + cap if text_cap is None else int(text_cap)) if gather else 0
    hits = np.zeros(cap, dtype=np.uint64)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    text = np.zeros(max(room, 1), dtype=np.uint8)
    offsets = np.zeros(cap + 1, dtype=np.uint64)
    lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().pire_hip_affix_lines_gather(_table_ptr(head), head_opts, _table_ptr(tail), tail_opts, raw.ctypes.data if raw.size else None,
                                             raw.size, delim, part, 0, _tail(delim if tail_byte == -1 else tail_byte), C.byref(lines),
                                             hits.ctypes.data if cap else None, spans.ctypes.data if cap else None, cap, C.byref(cnt),
                                             text.ctypes.data if room else None, room, offsets.ctypes.data if gather else None,
                                             C.byref(total) if gather else None, None))
    k = min(int(cnt.value), cap)
    out = {"lines": int(lines.value), "hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}
    if gather:
        out.update(text=text[:min(int(total.value), room)], offsets=offsets[:k + 1], bytes=int(total.value))
    return out


def affix_lines_gather_device(head, tail, raw_ptr: int, size: int, out_line_count_ptr: int, out_hit_count_ptr: int, part=AFFIX_HEAD,
                              out_bytes_ptr=0, delim: int = 10, head_opts=AFFIX_LONGEST, tail_opts=AFFIX_LONGEST, tail_byte=-1,
                              out_hits_ptr=0, out_spans_ptr=0, hit_cap=0, out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
    """pire_hip_affix_lines_gather on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
    _check(lib().pire_hip_affix_lines_gather(_table_ptr(head), head_opts, _table_ptr(tail), tail_opts, raw_ptr or None, size, delim, part,
                                             FLAG_ON_DEVICE, _tail(delim if tail_byte == -1 else tail_byte), out_line_count_ptr or None,
                                             out_hits_ptr or None, out_spans_ptr or None, hit_cap, out_hit_count_ptr or None,
                                             out_text_ptr or None, text_cap, out_offsets_ptr or None, out_bytes_ptr or None, stream or None))


# --- where the match lies: leftmost-longest spans (pire_hip_search and the forms on top of it).  rev: the Table of the
# reversed `(re).*`, fwd: the Table of `re`.
def search_opts(shortest=False, through_begin=False, through_end=False) -> int:
    """the PIRE_HIP_SEARCH_* bits"""
    return (SEARCH_SHORTEST if shortest else 0) | (SEARCH_THROUGH_BEGIN if through_begin else 0) | (SEARCH_THROUGH_END if through_end else 0)


def search(rev, fwd, text, offsets, opts=0):
    """pire_hip_search on host strings: (begin i64[n], end i64[n])."""
    text = _raw_bytes(text)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    begin, end = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    _check(lib().pire_hip_search(_table_ptr(rev), _table_ptr(fwd), opts, text.ctypes.data if text.size else None, offsets.ctypes.data, n, 0,
                                 begin.ctypes.data, end.ctypes.data, None))
    return begin, end


def search_device(rev, fwd, text_ptr: int, offsets_ptr: int, n: int, out_begin_ptr: int, out_end_ptr: int, opts=0, stream: int = 0):
    """pire_hip_search on device pointers: only enqueues on `stream`."""
    _check(lib().pire_hip_search(_table_ptr(rev), _table_ptr(fwd), opts, text_ptr or None, offsets_ptr or None, n, FLAG_ON_DEVICE,
                                 out_begin_ptr or None, out_end_ptr or None, stream or None))


def search_run_select(rev, fwd, text, offsets, opts=0, hit_cap: Optional[int] = None, positions=True):
    """pire_hip_search_run_select on host strings: {"hits", "spans", "count"} and, with positions, {"begin", "end"}; without,
    the library keeps those arrays to itself."""
    text = _raw_bytes(text)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    cap = n if hit_cap is None else int(hit_cap)
    begin = np.empty(n, dtype=np.int64) if positions else None
    end = np.empty(n, dtype=np.int64) if positions else None
    hits = np.zeros(cap, dtype=np.uint64)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_search_run_select(_table_ptr(rev), _table_ptr(fwd), opts, text.ctypes.data if text.size else None, offsets.ctypes.data,
                                            n, 0, _np_ptr(begin), _np_ptr(end), hits.ctypes.data if cap else None,
                                            spans.ctypes.data if cap else None, cap, C.byref(cnt), None))
    k = min(int(cnt.value), cap)
    out = {"hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}
    if positions:
        out.update(begin=begin, end=end)
    return out


def search_run_select_device(rev, fwd, text_ptr: int, offsets_ptr: int, n: int, out_hit_count_ptr: int, opts=0, out_begin_ptr=0,
                             out_end_ptr=0, out_hits_ptr=0, out_spans_ptr=0, hit_cap=0, stream: int = 0):
    """pire_hip_search_run_select on device pointers: only enqueues on `stream`."""
    _check(lib().pire_hip_search_run_select(_table_ptr(rev), _table_ptr(fwd), opts, text_ptr or None, offsets_ptr or None, n, FLAG_ON_DEVICE,
                                            out_begin_ptr or None, out_end_ptr or None, out_hits_ptr or None, out_spans_ptr or None, hit_cap,
                                            out_hit_count_ptr or None, stream or None))


def search_lines_gather_host(rev, fwd, raw, opts=0, delim: int = 10, tail_byte=-1, hit_cap=None, text_cap=None, gather=True):
    """pire_hip_search_lines_gather on a host buffer: {"lines", "hits", "spans", "count"} and, with gather, {"text", "offsets",
    "bytes"}.  tail_byte -1 = the delimiter, None = none; hit_cap None = room for a hit on every line, text_cap None = for all
    of them."""
    raw = _raw_bytes(raw)
    cap = raw.size if hit_cap is None else int(hit_cap)
    room = (raw.size + cap if text_cap is None else int(text_cap)) if gather else 0
    hits = np.zeros(cap, dtype=np.uint64)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    text = np.zeros(max(room, 1), dtype=np.uint8)
    offsets = np.zeros(cap + 1, dtype=np.uint64)
    lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().pire_hip_search_lines_gather(_table_ptr(rev), _table_ptr(fwd), opts, raw.ctypes.data if raw.size else None, raw.size, delim, 0,
                                              _tail(delim if tail_byte == -1 else tail_byte), C.byref(lines),
                                              hits.ctypes.data if cap else None, spans.ctypes.data if cap else None, cap, C.byref(cnt),
                                              text.ctypes.data if room else None, room, offsets.ctypes.data if gather else None,
                                              C.byref(total) if gather else None, None))
    k = min(int(cnt.value), cap)
    out = {"lines": int(lines.value), "hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}
    if gather:
        out.update(text=text[:min(int(total.value), room)], offsets=offsets[:k + 1], bytes=int(total.value))
    return out


def search_lines_gather_device(rev, fwd, raw_ptr: int, size: int, out_line_count_ptr: int, out_hit_count_ptr: int, opts=0, out_bytes_ptr=0,
                               delim: int = 10, tail_byte=-1, out_hits_ptr=0, out_spans_ptr=0, hit_cap=0, out_text_ptr=0, text_cap=0,
                               out_offsets_ptr=0, stream: int = 0):
    """pire_hip_search_lines_gather on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
    _check(lib().pire_hip_search_lines_gather(_table_ptr(rev), _table_ptr(fwd), opts, raw_ptr or None, size, delim, FLAG_ON_DEVICE,
                                              _tail(delim if tail_byte == -1 else tail_byte), out_line_count_ptr or None,
                                              out_hits_ptr or None, out_spans_ptr or None, hit_cap, out_hit_count_ptr or None,
                                              out_text_ptr or None, text_cap, out_offsets_ptr or None, out_bytes_ptr or None, stream or None))


def search_all(rev, fwd, text, offsets, opts=0, match_cap: Optional[int] = None, text_bytes: Optional[int] = None, want_rows=True,
               want_owners=True, want_spans=True):
    """pire_hip_search_all on host strings: {"rows" u64[n + 1], "owners" u64[k], "spans" u64[k, 2], "count"}, k = min(count,
    match_cap); an output that is not wanted is None.  match_cap None = room for a match at every byte; text_bytes None = the
    size of `text`."""
    text = _raw_bytes(text)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    cap = text.size if match_cap is None else int(match_cap)
    rows = np.zeros(n + 1, dtype=np.uint64) if want_rows else None
    owners = np.zeros(cap, dtype=np.uint64) if want_owners and cap else None
    spans = np.zeros((cap, 2), dtype=np.uint64) if want_spans and cap else None
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_search_all(_table_ptr(rev), _table_ptr(fwd), opts, text.ctypes.data if text.size else None,
                                     text.size if text_bytes is None else int(text_bytes), offsets.ctypes.data, n, 0, _np_ptr(rows),
                                     _np_ptr(owners), _np_ptr(spans), cap, C.byref(cnt), None))
    k = min(int(cnt.value), cap)
    return {"rows": rows, "owners": None if owners is None else owners[:k], "spans": None if spans is None else spans[:k],
            "count": int(cnt.value)}


def search_all_device(rev, fwd, text_ptr: int, text_bytes: int, offsets_ptr: int, n: int, out_match_count_ptr: int, opts=0, out_rows_ptr=0,
                      out_owners_ptr=0, out_spans_ptr=0, match_cap=0, stream: int = 0):
    """pire_hip_search_all on device pointers: only enqueues on `stream`."""
    _check(lib().pire_hip_search_all(_table_ptr(rev), _table_ptr(fwd), opts, text_ptr or None, text_bytes, offsets_ptr or None, n,
                                     FLAG_ON_DEVICE, out_rows_ptr or None, out_owners_ptr or None, out_spans_ptr or None, match_cap,
                                     out_match_count_ptr or None, stream or None))


def search_all_lines_gather_host(rev, fwd, raw, opts=0, delim: int = 10, tail_byte=-1, match_cap=None, text_cap=None, gather=True):
    """pire_hip_search_all_lines_gather on a host buffer: {"lines", "owners", "spans", "count"} and, with gather, {"text",
    "offsets", "bytes"}.  tail_byte -1 = the delimiter, None = none; match_cap None = room for a match at every byte, text_cap
    None = for all of them."""
    raw = _raw_bytes(raw)
    cap = raw.size if match_cap is None else int(match_cap)
    room = (raw.size + cap if text_cap is None else int(text_cap)) if gather else 0
    owners = np.zeros(cap, dtype=np.uint64)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    text = np.zeros(max(room, 1), dtype=np.uint8)
    offsets = np.zeros(cap + 1, dtype=np.uint64)
    lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().pire_hip_search_all_lines_gather(_table_ptr(rev), _table_ptr(fwd), opts, raw.ctypes.data if raw.size else None, raw.size, delim,
                                                  0, _tail(delim if tail_byte == -1 else tail_byte), C.byref(lines),
                                                  owners.ctypes.data if cap else None, spans.ctypes.data if cap else None, cap,
                                                  C.byref(cnt), text.ctypes.data if room else None, room,
                                                  offsets.ctypes.data if gather else None, C.byref(total) if gather else None, None))
    k = min(int(cnt.value), cap)
    out = {"lines": int(lines.value), "owners": owners[:k], "spans": spans[:k], "count": int(cnt.value)}
    if gather:
        out.update(text=text[:min(int(total.value), room)], offsets=offsets[:k + 1], bytes=int(total.value))
    return out


def search_all_lines_gather_device(rev, fwd, raw_ptr: int, size: int, out_line_count_ptr: int, out_match_count_ptr: int, opts=0,
                                   out_bytes_ptr=0, delim: int = 10, tail_byte=-1, out_owners_ptr=0, out_spans_ptr=0, match_cap=0,
                                   out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
    """pire_hip_search_all_lines_gather on device pointers (synchronises `stream` once, as search_lines_gather_device does)."""
    _check(lib().pire_hip_search_all_lines_gather(_table_ptr(rev), _table_ptr(fwd), opts, raw_ptr or None, size, delim, FLAG_ON_DEVICE,
                                                  _tail(delim if tail_byte == -1 else tail_byte), out_line_count_ptr or None,
                                                  out_owners_ptr or None, out_spans_ptr or None, match_cap, out_match_count_ptr or None,
                                                  out_text_ptr or None, text_cap, out_offsets_ptr or None, out_bytes_ptr or None,
                                                  stream or None))


def lex_labels(masks) -> np.ndarray:
    """u32 per entry: the lowest regexp of its mask (lex's first-rule-wins), LEX_GAP for a gap"""
    m = np.ascontiguousarray(masks, dtype=np.uint64)
    low = m & (~m + np.uint64(1))
    out = np.full(m.shape, LEX_GAP, dtype=np.uint32)
    nz = low != 0
    out[nz] = np.log2(low[nz].astype(np.float64)).astype(np.uint32)   # (a power of two: exact)
    return out


def lex(rev, fwd, text, offsets, opts=0, match_cap: Optional[int] = None, text_bytes: Optional[int] = None, want_rows=True,
        want_owners=True, want_spans=True, want_masks=True, want_label_counts=True):
    """pire_hip_lex on host strings: {"rows" u64[n + 1], "owners" u64[k], "spans" u64[k, 2], "masks" u64[k], "label_counts"
    u64[R + 1], "count"}, k = min(count, match_cap); an output that is not wanted is None.  rev may be None with LEX_TOKENS.
    match_cap None = room for an entry at every byte; text_bytes None = the size of `text`."""
    text = _raw_bytes(text)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    cap = text.size if match_cap is None else int(match_cap)
    rows = np.zeros(n + 1, dtype=np.uint64) if want_rows else None
    owners = np.zeros(cap, dtype=np.uint64) if want_owners and cap else None
    spans = np.zeros((cap, 2), dtype=np.uint64) if want_spans and cap else None
    masks = np.zeros(cap, dtype=np.uint64) if want_masks and cap else None
    labels = np.zeros(fwd.info.regexps + 1, dtype=np.uint64) if want_label_counts and fwd is not None else None
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_lex(_table_ptr(rev), _table_ptr(fwd), opts, text.ctypes.data if text.size else None,
                              text.size if text_bytes is None else int(text_bytes), offsets.ctypes.data, n, 0, _np_ptr(rows), _np_ptr(owners),
                              _np_ptr(spans), _np_ptr(masks), cap, C.byref(cnt), _np_ptr(labels), None))
    k = min(int(cnt.value), cap)
    return {"rows": rows, "owners": None if owners is None else owners[:k], "spans": None if spans is None else spans[:k],
            "masks": None if masks is None else masks[:k], "label_counts": labels, "count": int(cnt.value)}


def lex_device(rev, fwd, text_ptr: int, text_bytes: int, offsets_ptr: int, n: int, out_match_count_ptr: int, opts=0, out_rows_ptr=0,
               out_owners_ptr=0, out_spans_ptr=0, out_masks_ptr=0, match_cap=0, out_label_counts_ptr=0, stream: int = 0):
    """pire_hip_lex on device pointers: only enqueues on `stream`."""
    _check(lib().pire_hip_lex(_table_ptr(rev), _table_ptr(fwd), opts, text_ptr or None, text_bytes, offsets_ptr or None, n, FLAG_ON_DEVICE,
                              out_rows_ptr or None, out_owners_ptr or None, out_spans_ptr or None, out_masks_ptr or None, match_cap,
                              out_match_count_ptr or None, out_label_counts_ptr or None, stream or None))


def lex_lines_gather_host(rev, fwd, raw, opts=0, delim: int = 10, tail_byte=-1, match_cap=None, text_cap=None, gather=True):
    """pire_hip_lex_lines_gather on a host buffer: {"lines", "owners", "spans", "masks", "label_counts", "count"} and, with
    gather, {"text", "offsets", "bytes"}.  tail_byte -1 = the delimiter, None = none; match_cap None = room for an entry at every
    byte, text_cap None = for all of them."""
    raw = _raw_bytes(raw)
    cap = raw.size if match_cap is None else int(match_cap)
    room = (raw.size + cap if text_cap is None else int(text_cap)) if gather else 0
    owners = np.zeros(cap, dtype=np.uint64)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    masks = np.zeros(cap, dtype=np.uint64)
    labels = np.zeros(fwd.info.regexps + 1, dtype=np.uint64)
    text = np.zeros(max(room, 1), dtype=np.uint8)
    offsets = np.zeros(cap + 1, dtype=np.uint64)
    lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().pire_hip_lex_lines_gather(_table_ptr(rev), _table_ptr(fwd), opts, raw.ctypes.data if raw.size else None, raw.size, delim, 0,
                                           _tail(delim if tail_byte == -1 else tail_byte), C.byref(lines),
                                           owners.ctypes.data if cap else None, spans.ctypes.data if cap else None,
                                           masks.ctypes.data if cap else None, cap, C.byref(cnt), labels.ctypes.data,
                                           text.ctypes.data if room else None, room, offsets.ctypes.data if gather else None,
                                           C.byref(total) if gather else None, None))
    k = min(int(cnt.value), cap)
    out = {"lines": int(lines.value), "owners": owners[:k], "spans": spans[:k], "masks": masks[:k], "label_counts": labels,
           "count": int(cnt.value)}
    if gather:
        out.update(text=text[:min(int(total.value), room)], offsets=offsets[:k + 1], bytes=int(total.value))
    return out


def lex_lines_gather_device(rev, fwd, raw_ptr: int, size: int, out_line_count_ptr: int, out_match_count_ptr: int, opts=0, out_bytes_ptr=0,
                            delim: int = 10, tail_byte=-1, out_owners_ptr=0, out_spans_ptr=0, out_masks_ptr=0, match_cap=0,
                            out_label_counts_ptr=0, out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
    """pire_hip_lex_lines_gather on device pointers (synchronises `stream` once, as search_all_lines_gather_device does)."""
    _check(lib().pire_hip_lex_lines_gather(_table_ptr(rev), _table_ptr(fwd), opts, raw_ptr or None, size, delim, FLAG_ON_DEVICE,
                                           _tail(delim if tail_byte == -1 else tail_byte), out_line_count_ptr or None, out_owners_ptr or None,
                                           out_spans_ptr or None, out_masks_ptr or None, match_cap, out_match_count_ptr or None,
                                           out_label_counts_ptr or None, out_text_ptr or None, text_cap, out_offsets_ptr or None,
                                           out_bytes_ptr or None, stream or None))


def splice(raw, spans, head=b"", tail=b"", mode=0, offsets=None, text_cap: Optional[int] = None, want_pos=True):
    """pire_hip_splice on host arrays: {"text" u8[min(bytes, text_cap)], "bytes", "pos" u64[k] or None, "offsets" u64[n + 1] or
    None}.  spans: u64[k, 2], ascending and disjoint; head, tail: bytes, at most SPLICE_PIECE_MAX each; text_cap None = room
    for the whole result."""
    raw = _raw_bytes(raw)
    spans = np.ascontiguousarray(spans, dtype=np.uint64).reshape(-1, 2)
    head, tail = bytes(head), bytes(tail)
    k = spans.shape[0]
    grown = k * (len(head) + len(tail)) - (0 if mode & SPLICE_KEEP else int((spans[:, 1] - spans[:, 0]).sum()))
    room = max(raw.size + grown, 0) if text_cap is None else int(text_cap)
    offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    out_offs = None if offs is None else np.zeros(offs.size, dtype=np.uint64)
    pos = np.zeros(k, dtype=np.uint64) if want_pos and k else None
    text = np.zeros(max(room, 1), dtype=np.uint8)
    total = C.c_uint64(0)
    _check(lib().pire_hip_splice(raw.ctypes.data if raw.size else None, raw.size, spans.ctypes.data if k else None, None, k,
                                 head or None, len(head), tail or None, len(tail), mode, _np_ptr(offs), 0 if offs is None else offs.size - 1, 0,
                                 text.ctypes.data if room else None, room, _np_ptr(pos), _np_ptr(out_offs), C.byref(total), None))
    return {"text": text[:min(int(total.value), room)], "bytes": int(total.value), "pos": pos, "offsets": out_offs}


def splice_device(raw_ptr: int, size: int, spans_ptr: int, span_cap: int, out_bytes_ptr: int, head=b"", tail=b"", mode=0, span_count_ptr=0,
                  offsets_ptr=0, n=0, out_text_ptr=0, text_cap=0, out_pos_ptr=0, out_offsets_ptr=0, stream: int = 0):
    """pire_hip_splice on device pointers (head and tail are host bytes in every mode): only enqueues on `stream`."""
    head, tail = bytes(head), bytes(tail)
    _check(lib().pire_hip_splice(raw_ptr or None, size, spans_ptr or None, span_count_ptr or None, span_cap, head or None, len(head),
                                 tail or None, len(tail), mode, offsets_ptr or None, n, FLAG_ON_DEVICE, out_text_ptr or None, text_cap,
                                 out_pos_ptr or None, out_offsets_ptr or None, out_bytes_ptr or None, stream or None))


def search_lines_splice_host(rev, fwd, raw, head=b"", tail=b"", mode=0, opts=0, delim: int = 10, match_cap=None, text_cap=None):
    """pire_hip_search_lines_splice on a host buffer: {"lines", "count", "spans" u64[k, 2], "pos" u64[k], "text", "bytes"}, k =
    min(count, match_cap).  match_cap None = room for a match at every byte (and one more: an insertion at the end); text_cap
    None = for all of them."""
    raw = _raw_bytes(raw)
    head, tail = bytes(head), bytes(tail)
    cap = raw.size + 1 if match_cap is None else int(match_cap)
    room = raw.size + cap * (len(head) + len(tail)) if text_cap is None else int(text_cap)
    spans = np.zeros((cap, 2), dtype=np.uint64)
    pos = np.zeros(cap, dtype=np.uint64)
    text = np.zeros(max(room, 1), dtype=np.uint8)
    lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().pire_hip_search_lines_splice(_table_ptr(rev), _table_ptr(fwd), opts, raw.ctypes.data if raw.size else None, raw.size, delim, 0,
                                              head or None, len(head), tail or None, len(tail), mode, C.byref(lines),
                                              spans.ctypes.data if cap else None, pos.ctypes.data if cap else None, cap, C.byref(cnt),
                                              text.ctypes.data if room else None, room, C.byref(total), None))
    k = min(int(cnt.value), cap)
    return {"lines": int(lines.value), "count": int(cnt.value), "spans": spans[:k], "pos": pos[:k],
            "text": text[:min(int(total.value), room)], "bytes": int(total.value)}


def search_lines_splice_device(rev, fwd, raw_ptr: int, size: int, out_line_count_ptr: int, out_match_count_ptr: int, out_bytes_ptr: int,
                               head=b"", tail=b"", mode=0, opts=0, delim: int = 10, out_spans_ptr=0, out_pos_ptr=0, match_cap=0,
                               out_text_ptr=0, text_cap=0, stream: int = 0):
    """pire_hip_search_lines_splice on device pointers (synchronises `stream` once, as search_lines_gather_device does)."""
    head, tail = bytes(head), bytes(tail)
    _check(lib().pire_hip_search_lines_splice(_table_ptr(rev), _table_ptr(fwd), opts, raw_ptr or None, size, delim, FLAG_ON_DEVICE,
                                              head or None, len(head), tail or None, len(tail), mode, out_line_count_ptr or None,
                                              out_spans_ptr or None, out_pos_ptr or None, match_cap, out_match_count_ptr or None,
                                              out_text_ptr or None, text_cap, out_bytes_ptr or None, stream or None))


def capture_select_host(offsets, begin, end, final=None, flags=FLAG_BEGIN, need_final=False, hit_cap: Optional[int] = None,
                        want_hits=True, want_spans=True):
    """pire_hip_capture_select on host arrays: (hits u64[k] or None, spans u64[k, 2] or None, count), k = min(count, hit_cap).
    flags: FLAG_BEGIN where the capture call had it; hit_cap None = room for every string."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    begin = np.ascontiguousarray(begin, dtype=np.int64)
    end = np.ascontiguousarray(end, dtype=np.int64)
    final = None if final is None else np.ascontiguousarray(final, dtype=np.uint8)
    n = len(offsets) - 1
    cap = n if hit_cap is None else int(hit_cap)
    hits = np.zeros(cap, dtype=np.uint64) if want_hits else None
    spans = np.zeros((cap, 2), dtype=np.uint64) if want_spans else None
    cnt = C.c_uint64(0)
    _check(lib().pire_hip_capture_select(offsets.ctypes.data, n, flags & FLAG_BEGIN, begin.ctypes.data if n else None,
                                         end.ctypes.data if n else None, _np_ptr(final), int(bool(need_final)),
                                         _np_ptr(hits) if cap else None, _np_ptr(spans) if cap else None, cap, C.byref(cnt), None))
    k = min(int(cnt.value), cap)
    return (None if hits is None else hits[:k]), (None if spans is None else spans[:k]), int(cnt.value)


def capture_select_device(offsets_ptr: int, n: int, flags, begin_ptr: int, end_ptr: int, out_hit_count_ptr: int, final_ptr=0,
                          need_final=False, out_hits_ptr=0, out_spans_ptr=0, hit_cap=0, stream: int = 0):
    """pire_hip_capture_select with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
    _check(lib().pire_hip_capture_select(offsets_ptr or None, n, (flags & FLAG_BEGIN) | FLAG_ON_DEVICE, begin_ptr or None,
                                         end_ptr or None, final_ptr or None, int(bool(need_final)), out_hits_ptr or None,
                                         out_spans_ptr or None, hit_cap, out_hit_count_ptr or None, stream or None))


class Table:
    """An ingested Pire::Scanner / NonrelocScanner / SimpleScanner (from Save() bytes).  Mirrors the public getters."""

    def __init__(self, blob: bytes = None, _handle=None):
        L = lib()
        h = _handle
        if h is None:
            h = C.c_void_p()
            blob = bytes(blob)
            _check(L.pire_hip_table_create(blob, len(blob), C.byref(h)))
        self._h = h
        self._info = None

    @property
    def info(self):
        """pire_hip_table_info (fetched on first use: for a glued table it triggers the dense-row ranking)."""
        if self._info is None:
            info = TableInfo()
            _check(lib().pire_hip_table_get_info(self._h, C.byref(info)))
            self._info = info
        return self._info

    @classmethod
    def from_file(cls, path: str):
        """Scanner::Mmap deployment flow (samples/blacklist/blacklist.cpp:86-93): ingest a file written by Save()."""
        h = C.c_void_p()
        _check(lib().pire_hip_table_create_from_file(os.fsencode(path), C.byref(h)))
        return cls(_handle=h)

    @classmethod
    def mmap(cls, image: bytes):
        """Ingest the scanner at the start of `image`; returns (table, bytes consumed) like Scanner::Mmap's pointer."""
        h = C.c_void_p()
        used = C.c_size_t()
        image = bytes(image)
        _check(lib().pire_hip_table_mmap(image, len(image), C.byref(h), C.byref(used)))
        return cls(_handle=h), used.value

    @classmethod
    def glue(cls, lhs: "Table", rhs: "Table", max_size: int = 0, gpu: bool = False):
        """Scanner::Glue(lhs, rhs, maxSize) on two ingested tables (reference numbering); gpu=True: BFS on the device."""
        for t in (lhs, rhs):
            if not isinstance(t, Table):   # a CountingTable's or SlowTable's handle is another C type: never hand it over
                raise PireHipError(-1, "Glue is defined for Pire::Scanner tables, not for a %s" % type(t).__name__)
        h = C.c_void_p()
        fn = lib().pire_hip_table_glue_gpu if gpu else lib().pire_hip_table_glue
        _check(fn(lhs._h, rhs._h, max_size, C.byref(h)))
        return cls(_handle=h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:      # at interpreter shutdown the module globals may already be gone
            try:
                _lib.pire_hip_table_destroy(h)
            except Exception:
                pass
            self._h = None

    # --- Scanner getters (multi.h:134-161)
    Size = property(lambda s: s.info.states)
    LettersCount = property(lambda s: s.info.letters)
    RegexpsCount = property(lambda s: s.info.regexps)
    Empty = property(lambda s: bool(s.info.empty))
    initial = property(lambda s: s.info.initial)

    def refresh_info(self):
        self._info = None
        return self.info

    def Final(self, idx: int) -> bool:
        return bool(_check(lib().pire_hip_table_final(self._h, idx)))

    def Dead(self, idx: int) -> bool:
        return bool(_check(lib().pire_hip_table_dead(self._h, idx)))

    def AcceptedRegexps(self, idx: int):
        b = u64p()
        n = C.c_size_t()
        _check(lib().pire_hip_table_accepted_regexps(self._h, idx, C.byref(b), C.byref(n)))
        return [int(b[i]) for i in range(n.value)]

    def letter_class(self, ch: int) -> int:
        return _check(lib().pire_hip_table_letter_class(self._h, ch))

    def Next(self, idx: int, ch: int) -> int:
        """Table accessor (Scanner::Next on indices); not a scan loop."""
        return _check(lib().pire_hip_table_next(self._h, idx, ch))

    def layout(self):
        """(orig_of_perm u32[states], hot_rows u8[hot+1, 256]) -- the device numbering and dense LDS rows."""
        o = np.empty(self.info.states, dtype=np.uint32)
        h = np.empty((self.info.hot_states + 1, 256), dtype=np.uint8)
        _check(lib().pire_hip_table_layout(self._h, o.ctypes.data, h.ctypes.data))
        return o, h

    def wide_layout(self):
        """(rows u16[wide + 1, pitch / 2], wide_states, pitch, rows_offset): the class-indexed walk's LDS image (wide.hip);
        rows is None for a table that fits the dense rows."""
        w, pitch, off = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().pire_hip_table_wide_layout(self._h, None, 0, C.byref(w), C.byref(pitch), C.byref(off)))
        if not w.value:
            return None, 0, pitch.value, off.value
        rows = np.empty((w.value + 1, pitch.value // 2), dtype=np.uint16)
        _check(lib().pire_hip_table_wide_layout(self._h, rows.ctypes.data, rows.size, C.byref(w), C.byref(pitch), C.byref(off)))
        return rows, w.value, pitch.value, off.value

    def zip_layout(self):
        """None, or the ZIPPED image of the class-indexed walk (pire_hip_table_zip_layout): a dict with tier, full, pitch,
        rows_offset and the decoded pieces rows u16[full + 1, pitch / 2], headers u32[tier + 1], targets u16[tier - full, 3]."""
        g = (C.c_uint32 * 8)()
        _check(lib().pire_hip_table_zip_layout(self._h, None, 0, g))
        tier, full, pitch, rows_off, h_off, x_off, end, k = list(g)
        if not full:
            return None
        img = np.empty((end - rows_off) // 2, dtype=np.uint16)
        _check(lib().pire_hip_table_zip_layout(self._h, img.ctypes.data, img.size, g))
        raw = img.view(np.uint8)
        rows = raw[:(full + 1) * pitch].view(np.uint16).reshape(full + 1, pitch // 2)
        headers = raw[h_off - rows_off:h_off - rows_off + 4 * (tier + 1)].view(np.uint32)
        targets = raw[x_off - rows_off:x_off - rows_off + 2 * k * (tier - full)].view(np.uint16).reshape(tier - full, k)
        return {"tier": tier, "full": full, "pitch": pitch, "rows_offset": rows_off, "rows": rows, "headers": headers,
                "targets": targets}

    def set_config(self, **fields):
        """pire_hip_table_config_set: this table's own configuration = the current one with `fields` changed; no fields: back to the
        process-wide configuration."""
        if not fields:
            _check(lib().pire_hip_table_config_set(self._h, None))
            return None
        c = self.get_config()
        for k, v in fields.items():
            setattr(c, k, v)
        c.size = C.sizeof(Config)
        _check(lib().pire_hip_table_config_set(self._h, C.byref(c)))
        return c

    def get_config(self) -> "Config":
        c = Config()
        c.size = C.sizeof(Config)
        _check(lib().pire_hip_table_config_get(self._h, C.byref(c)))
        return c

    def adapt(self) -> int:
        """Re-rank the LDS rows from the visit counters of earlier scans; returns the number of rows promoted."""
        n = C.c_uint32(0)
        _check(lib().pire_hip_table_adapt(self._h, C.byref(n)))
        self.refresh_info()
        return n.value

    def upload(self):
        _check(lib().pire_hip_table_upload(self._h))

    # --- host-pointer runs (numpy in, numpy out): the PCIe-inclusive convenience mode
    def run(self, text, offsets, flags=FLAG_BEGIN | FLAG_END, init_idx=None, counts=False):
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        idx = np.empty(n, dtype=np.uint32)
        fin = np.empty(n, dtype=np.uint8)
        init = None if init_idx is None else np.ascontiguousarray(init_idx, dtype=np.uint32)
        cnt = np.zeros(self.RegexpsCount + 2, dtype=np.uint64) if counts else None
        _check(lib().pire_hip_run(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                  flags & ~FLAG_ON_DEVICE, _np_ptr(init), idx.ctypes.data, fin.ctypes.data,
                                  _np_ptr(cnt), None))
        return (idx, fin, cnt) if counts else (idx, fin)

    def run_strings(self, strings, **kw):
        offs = np.zeros(len(strings) + 1, dtype=np.uint64)
        if strings:
            offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        text = np.frombuffer(b"".join(strings), dtype=np.uint8)
        return self.run(text, offs, **kw)

    def run_strided_host(self, text2d: np.ndarray, flags=FLAG_BEGIN | FLAG_END, init_idx=None, counts=False):
        text2d = np.ascontiguousarray(text2d, dtype=np.uint8)
        n, length = text2d.shape
        idx = np.empty(n, dtype=np.uint32)
        fin = np.empty(n, dtype=np.uint8)
        init = None if init_idx is None else np.ascontiguousarray(init_idx, dtype=np.uint32)
        cnt = np.zeros(self.RegexpsCount + 2, dtype=np.uint64) if counts else None
        _check(lib().pire_hip_run_strided(self._h, text2d.ctypes.data if text2d.size else None, n, length, length,
                                          flags & ~FLAG_ON_DEVICE, _np_ptr(init), idx.ctypes.data, fin.ctypes.data,
                                          _np_ptr(cnt), None))
        return (idx, fin, cnt) if counts else (idx, fin)

    # --- device-pointer runs (raw addresses; torch tensors' data_ptr()): only enqueue on `stream`
    def run_strided_device(self, text_ptr: int, n: int, length: int, stride: int, flags, out_idx_ptr=0,
                           out_final_ptr=0, out_counts_ptr=0, init_ptr=0, stream: int = 0):
        _check(lib().pire_hip_run_strided(self._h, text_ptr or None, n, length, stride, flags | FLAG_ON_DEVICE,
                                          init_ptr or None, out_idx_ptr or None, out_final_ptr or None,
                                          out_counts_ptr or None, stream or None))

    def run_device_host_offsets(self, text_ptr: int, offsets: np.ndarray, flags, out_idx_ptr=0, out_final_ptr=0,
                                out_counts_ptr=0, init_ptr=0, stream: int = 0):
        """Resident text (device pointer), offsets on the host (PIRE_HIP_RUN_HOST_OFFSETS); outputs on the device."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _check(lib().pire_hip_run(self._h, text_ptr or None, offsets.ctypes.data, len(offsets) - 1,
                                  flags | FLAG_ON_DEVICE | FLAG_HOST_OFFSETS, init_ptr or None, out_idx_ptr or None,
                                  out_final_ptr or None, out_counts_ptr or None, stream or None))

    def run_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_idx_ptr=0, out_final_ptr=0,
                   out_counts_ptr=0, init_ptr=0, stream: int = 0):
        _check(lib().pire_hip_run(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                  init_ptr or None, out_idx_ptr or None, out_final_ptr or None,
                                  out_counts_ptr or None, stream or None))

    # --- which strings matched which regexps (pire_hip_select): masks are uint64[n, mask_words], hits ascending indices
    @property
    def mask_words(self) -> int:
        """W = max(1, ceil(RegexpsCount / 64)): 64-bit words of a regexp mask."""
        return int(lib().pire_hip_table_mask_words(self._h))

    def want_mask(self, want):
        """None, or uint64[mask_words] from an iterable of regexp numbers / an array that already is one."""
        if want is None:
            return None
        if isinstance(want, np.ndarray) and want.dtype == np.uint64:
            if want.size != self.mask_words:
                raise ValueError("want: %d words, the table's masks have %d" % (want.size, self.mask_words))
            return np.ascontiguousarray(want)
        m = np.zeros(self.mask_words, dtype=np.uint64)
        for r in want:
            if int(r) < 64 * self.mask_words:
                m[int(r) // 64] |= np.uint64(1 << (int(r) % 64))
        return m

    def _select_outputs(self, n, hit_cap, masks, hit_masks):
        cap = n if hit_cap is None else int(hit_cap)
        w = self.mask_words
        return (cap, np.zeros((n, w), dtype=np.uint64) if masks else None, np.zeros(cap, dtype=np.uint64),
                np.zeros((cap, w), dtype=np.uint64) if hit_masks else None, C.c_uint64(0))

    @staticmethod
    def _select_result(cap, om, oh, ohm, cnt):
        k = min(int(cnt.value), cap)
        return {"masks": om, "hits": oh[:k], "hit_masks": None if ohm is None else ohm[:k], "count": int(cnt.value)}

    def select(self, state_idx, want=None, hit_cap=None, masks=True, hit_masks=True):
        """pire_hip_select on host arrays: {"masks", "hits", "hit_masks", "count"}; hit_cap None = room for every string."""
        idx = np.ascontiguousarray(state_idx, dtype=np.uint32)
        wm = self.want_mask(want)
        cap, om, oh, ohm, cnt = self._select_outputs(len(idx), hit_cap, masks, hit_masks)
        _check(lib().pire_hip_select(self._h, idx.ctypes.data if idx.size else None, len(idx), _np_ptr(wm), 0, _np_ptr(om),
                                     oh.ctypes.data if cap else None, _np_ptr(ohm) if cap else None, cap, C.byref(cnt), None))
        return self._select_result(cap, om, oh, ohm, cnt)

    def run_select(self, text, offsets, flags=FLAG_BEGIN | FLAG_END, want=None, hit_cap=None, init_idx=None, masks=True,
                   hit_masks=True, states=True):
        """pire_hip_run_select on host arrays: select()'s dict plus "idx" / "final" of the scan (states=False: the library
        keeps the state indices to itself)."""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        idx = np.empty(n, dtype=np.uint32) if states else None
        fin = np.empty(n, dtype=np.uint8) if states else None
        init = None if init_idx is None else np.ascontiguousarray(init_idx, dtype=np.uint32)
        wm = self.want_mask(want)
        cap, om, oh, ohm, cnt = self._select_outputs(n, hit_cap, masks, hit_masks)
        _check(lib().pire_hip_run_select(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                         flags & ~FLAG_ON_DEVICE, _np_ptr(init), _np_ptr(idx), _np_ptr(fin), None, _np_ptr(wm),
                                         _np_ptr(om), oh.ctypes.data if cap else None, _np_ptr(ohm) if cap else None, cap,
                                         C.byref(cnt), None))
        out = self._select_result(cap, om, oh, ohm, cnt)
        out["idx"], out["final"] = idx, fin
        return out

    def select_device(self, state_idx_ptr: int, n: int, out_hit_count_ptr: int, want_ptr=0, out_masks_ptr=0, out_hits_ptr=0,
                      out_hit_masks_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_select with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
        _check(lib().pire_hip_select(self._h, state_idx_ptr or None, n, want_ptr or None, FLAG_ON_DEVICE, out_masks_ptr or None,
                                     out_hits_ptr or None, out_hit_masks_ptr or None, hit_cap, out_hit_count_ptr or None,
                                     stream or None))

    def run_select_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_hit_count_ptr: int, want_ptr=0,
                          out_masks_ptr=0, out_hits_ptr=0, out_hit_masks_ptr=0, hit_cap=0, out_idx_ptr=0, out_final_ptr=0,
                          out_counts_ptr=0, init_ptr=0, stream: int = 0):
        """pire_hip_run_select on device pointers (FLAG_HOST_OFFSETS in `flags`: offsets_ptr is a host address)."""
        _check(lib().pire_hip_run_select(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                         init_ptr or None, out_idx_ptr or None, out_final_ptr or None, out_counts_ptr or None,
                                         want_ptr or None, out_masks_ptr or None, out_hits_ptr or None,
                                         out_hit_masks_ptr or None, hit_cap, out_hit_count_ptr or None, stream or None))

    def run_select_strided_device(self, text_ptr: int, n: int, length: int, stride: int, flags, out_hit_count_ptr: int,
                                  want_ptr=0, out_masks_ptr=0, out_hits_ptr=0, out_hit_masks_ptr=0, hit_cap=0, out_idx_ptr=0,
                                  out_final_ptr=0, out_counts_ptr=0, init_ptr=0, stream: int = 0):
        """pire_hip_run_select_strided on device pointers: fixed-length records, only enqueues on `stream`."""
        _check(lib().pire_hip_run_select_strided(self._h, text_ptr or None, n, length, stride, flags | FLAG_ON_DEVICE,
                                                 init_ptr or None, out_idx_ptr or None, out_final_ptr or None,
                                                 out_counts_ptr or None, want_ptr or None, out_masks_ptr or None,
                                                 out_hits_ptr or None, out_hit_masks_ptr or None, hit_cap,
                                                 out_hit_count_ptr or None, stream or None))

    # --- raw bytes in, the matching lines out (pire_hip_run_lines_select): spans are uint64[hits, 2], begin / end in raw
    def run_lines_select_host(self, raw, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, want=None, hit_cap=None, hit_masks=True):
        """pire_hip_run_lines_select on a host buffer: {"lines", "hits", "spans", "hit_masks", "count"}; hit_cap None = room for
        a hit on every line (no more lines than bytes)."""
        raw = _raw_bytes(raw)
        wm = self.want_mask(want)
        cap = raw.size if hit_cap is None else int(hit_cap)
        w = self.mask_words
        hits = np.zeros(cap, dtype=np.uint64)
        spans = np.zeros((cap, 2), dtype=np.uint64)
        masks = np.zeros((cap, w), dtype=np.uint64) if hit_masks else None
        lines, cnt = C.c_uint64(0), C.c_uint64(0)
        _check(lib().pire_hip_run_lines_select(self._h, raw.ctypes.data if raw.size else None, raw.size, delim, flags & ~FLAG_ON_DEVICE,
                                               _np_ptr(wm), C.byref(lines), hits.ctypes.data if cap else None,
                                               spans.ctypes.data if cap else None, _np_ptr(masks) if cap else None, cap,
                                               C.byref(cnt), None))
        k = min(int(cnt.value), cap)
        return {"lines": int(lines.value), "hits": hits[:k], "spans": spans[:k], "hit_masks": None if masks is None else masks[:k],
                "count": int(cnt.value)}

    def run_lines_select_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int, delim: int = 10,
                                want_ptr=0, out_hits_ptr=0, out_hit_spans_ptr=0, out_hit_masks_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_run_lines_select on device pointers (synchronises `stream` once: the number of lines sizes its scratch)."""
        _check(lib().pire_hip_run_lines_select(self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, want_ptr or None,
                                               out_line_count_ptr or None, out_hits_ptr or None, out_hit_spans_ptr or None,
                                               out_hit_masks_ptr or None, hit_cap, out_hit_count_ptr or None, stream or None))

    # --- one ascending hit list per regexp (pire_hip_route): counts uint64[R], hits a list of R arrays (row r: the strings
    # that matched regexp r).  device=True: the same call with PIRE_HIP_RUN_ON_DEVICE on torch buffers (the inputs are copied
    # to the current device first, the rows fetched afterwards; "device_hits" int64[R, cap] and "device_counts" int64[R] stay
    # there for chaining); the *_device methods below take raw addresses and only enqueue.
    @staticmethod
    def _route_rows(counts, flat, cap, width=1):
        r = len(counts)
        rows = flat.reshape(r, cap, width) if width > 1 else flat.reshape(r, cap)
        return [rows[k, :min(int(counts[k]), cap)].copy() for k in range(r)]

    def _route_call(self, n, cap, device, call, spans=False):
        """call(hits_ptr, spans_ptr, counts_ptr, flag, stream) makes the C call; -> the result dict"""
        r = self.RegexpsCount
        if not device:
            counts = np.zeros(r, dtype=np.uint64)
            hits = np.zeros(max(r * cap, 1), dtype=np.uint64)
            sp = np.zeros(max(r * cap, 1) * 2, dtype=np.uint64) if spans else None
            call(hits.ctypes.data if cap else None, sp.ctypes.data if spans and cap else None, counts.ctypes.data if r else None,
                 0, None)
            out = {"counts": counts, "hits": self._route_rows(counts, hits[:r * cap], cap)}
            if spans:
                out["spans"] = self._route_rows(counts, sp[:r * cap * 2], cap, 2)
            return out
        import torch

        dc = torch.zeros(max(r, 1), dtype=torch.int64, device="cuda")
        dh = torch.zeros((max(r, 1), max(cap, 1)), dtype=torch.int64, device="cuda")
        ds = torch.zeros((max(r, 1), max(cap, 1), 2), dtype=torch.int64, device="cuda") if spans else None
        call(dh.data_ptr() if cap else None, ds.data_ptr() if spans and cap else None, dc.data_ptr() if r else None,
             FLAG_ON_DEVICE, torch.cuda.current_stream().cuda_stream or None)
        torch.cuda.synchronize()
        counts = dc.cpu().numpy().view(np.uint64)[:r].copy()
        out = {"counts": counts, "hits": self._route_rows(counts, dh.cpu().numpy().view(np.uint64)[:r, :cap].reshape(-1), cap),
               "device_hits": dh, "device_counts": dc}
        if spans:
            out["spans"] = self._route_rows(counts, ds.cpu().numpy().view(np.uint64)[:r, :cap].reshape(-1), cap, 2)
            out["device_spans"] = ds
        return out

    @staticmethod
    def _to_device(a):
        import torch

        a = np.ascontiguousarray(a)
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
        if a.size == 0:
            return torch.zeros(256, dtype=torch.uint8, device="cuda")
        return torch.as_tensor(a.view(signed) if signed else a, device="cuda")

    def route(self, state_idx, cap=None, device=False):
        """pire_hip_route: {"counts": u64[R], "hits": [R arrays]}; cap None = room for every string in every row."""
        idx = np.ascontiguousarray(state_idx, dtype=np.uint32)
        n = len(idx)
        cap = n if cap is None else int(cap)
        src = self._to_device(idx) if device else idx
        ptr = (src.data_ptr() if device else idx.ctypes.data) if n else None

        def call(hits, _spans, counts, flag, stream):
            _check(lib().pire_hip_route(self._h, ptr, n, flag, hits, cap, counts, stream))
        return self._route_call(n, cap, device, call)

    def run_route(self, text, offsets, flags=FLAG_BEGIN | FLAG_END, cap=None, init_idx=None, states=True, device=False):
        """pire_hip_run_route: route()'s dict plus "idx" / "final" of the scan (states=False: the library keeps the state
        indices to itself)."""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        return self._run_route(n, cap, init_idx, states, device, flags, (text, offsets), None)

    def run_route_strided(self, text2d, flags=FLAG_BEGIN | FLAG_END, cap=None, init_idx=None, states=True, device=False):
        """pire_hip_run_route_strided on fixed-length records uint8[n, len]: run_route()'s dict."""
        text2d = np.ascontiguousarray(text2d, dtype=np.uint8)
        return self._run_route(text2d.shape[0], cap, init_idx, states, device, flags, None, text2d)

    def _run_route(self, n, cap, init_idx, states, device, flags, batch, records):
        cap = n if cap is None else int(cap)
        init = None if init_idx is None else np.ascontiguousarray(init_idx, dtype=np.uint32)
        flags &= ~FLAG_ON_DEVICE
        if device:
            import torch

            hold = [self._to_device(a) for a in (batch if records is None else (records,))]
            dinit = None if init is None else self._to_device(init)
            idx = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda") if states else None
            fin = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda") if states else None
            ptrs = [h.data_ptr() for h in hold]
            pinit, pidx, pfin = (None if x is None else x.data_ptr() for x in (dinit, idx, fin))
        else:
            idx = np.empty(n, dtype=np.uint32) if states else None
            fin = np.empty(n, dtype=np.uint8) if states else None
            if records is None:
                ptrs = [batch[0].ctypes.data if batch[0].size else None, batch[1].ctypes.data]
            else:
                ptrs = [records.ctypes.data if records.size else None]
            pinit, pidx, pfin = _np_ptr(init), _np_ptr(idx), _np_ptr(fin)

        def call(hits, _spans, counts, flag, stream):
            if records is None:
                _check(lib().pire_hip_run_route(self._h, ptrs[0], ptrs[1], n, flags | flag, pinit, pidx, pfin, None, hits, cap, counts,
                                                stream))
            else:
                _check(lib().pire_hip_run_route_strided(self._h, ptrs[0], n, records.shape[1], records.shape[1], flags | flag, pinit,
                                                        pidx, pfin, None, hits, cap, counts, stream))
        out = self._route_call(n, cap, device, call)
        if states and device:
            idx, fin = idx.cpu().numpy().view(np.uint32)[:n], fin.cpu().numpy()[:n]
        out["idx"], out["final"] = idx, fin
        return out

    def run_lines_route(self, raw, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, cap=None, device=False):
        """pire_hip_run_lines_route: {"lines", "counts": u64[R], "hits": [R arrays of line numbers], "spans": [R arrays u64[k, 2]]};
        cap None = room for a hit on every line (no more lines than bytes) in every row."""
        raw = _raw_bytes(raw)
        cap = raw.size if cap is None else int(cap)
        flags &= ~FLAG_ON_DEVICE
        if device:
            import torch

            src = self._to_device(raw)
            dn = torch.zeros(1, dtype=torch.int64, device="cuda")
            praw, pn = src.data_ptr() if raw.size else None, dn.data_ptr()
        else:
            lines = C.c_uint64(0)
            praw, pn = raw.ctypes.data if raw.size else None, C.addressof(lines)

        def call(hits, spans, counts, flag, stream):
            _check(lib().pire_hip_run_lines_route(self._h, praw, raw.size, delim, flags | flag, pn, hits, spans, cap, counts, stream))
        out = self._route_call(raw.size, cap, device, call, spans=True)
        out["lines"] = int(dn.cpu().numpy()[0]) if device else int(lines.value)
        return out

    def route_device(self, state_idx_ptr: int, n: int, out_hit_counts_ptr: int, out_hits_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_route with PIRE_HIP_RUN_ON_DEVICE: raw device addresses, only enqueues on `stream`."""
        _check(lib().pire_hip_route(self._h, state_idx_ptr or None, n, FLAG_ON_DEVICE, out_hits_ptr or None, hit_cap,
                                    out_hit_counts_ptr or None, stream or None))

    def run_route_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_hit_counts_ptr: int, out_hits_ptr=0, hit_cap=0,
                         out_idx_ptr=0, out_final_ptr=0, out_counts_ptr=0, init_ptr=0, stream: int = 0):
        """pire_hip_run_route on device pointers (FLAG_HOST_OFFSETS in `flags`: offsets_ptr is a host address)."""
        _check(lib().pire_hip_run_route(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE, init_ptr or None,
                                        out_idx_ptr or None, out_final_ptr or None, out_counts_ptr or None, out_hits_ptr or None,
                                        hit_cap, out_hit_counts_ptr or None, stream or None))

    def run_route_strided_device(self, text_ptr: int, n: int, length: int, stride: int, flags, out_hit_counts_ptr: int,
                                 out_hits_ptr=0, hit_cap=0, out_idx_ptr=0, out_final_ptr=0, out_counts_ptr=0, init_ptr=0,
                                 stream: int = 0):
        """pire_hip_run_route_strided on device pointers: fixed-length records, only enqueues on `stream`."""
        _check(lib().pire_hip_run_route_strided(self._h, text_ptr or None, n, length, stride, flags | FLAG_ON_DEVICE,
                                                init_ptr or None, out_idx_ptr or None, out_final_ptr or None,
                                                out_counts_ptr or None, out_hits_ptr or None, hit_cap,
                                                out_hit_counts_ptr or None, stream or None))

    def run_lines_route_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_hit_counts_ptr: int,
                               delim: int = 10, out_hits_ptr=0, out_hit_spans_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_run_lines_route on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
        _check(lib().pire_hip_run_lines_route(self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE,
                                              out_line_count_ptr or None, out_hits_ptr or None, out_hit_spans_ptr or None, hit_cap,
                                              out_hit_counts_ptr or None, stream or None))

    # --- raw bytes in, the matching lines out as bytes (pire_hip_run_lines_gather)
    def run_lines_gather_host(self, raw, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, want=None, tail=-1, hit_cap=None,
                              text_cap=None):
        """pire_hip_run_lines_gather on a host buffer: {"lines", "hits", "count", "text", "offsets", "bytes"}.  tail -1 = the
        delimiter (grep's output), None = none; hit_cap None = room for a hit on every line, text_cap None = for all of them."""
        raw = _raw_bytes(raw)
        wm = self.want_mask(want)
        cap = raw.size if hit_cap is None else int(hit_cap)
        room = raw.size + cap if text_cap is None else int(text_cap)
        hits = np.zeros(cap, dtype=np.uint64)
        text = np.zeros(max(room, 1), dtype=np.uint8)
        offsets = np.zeros(cap + 1, dtype=np.uint64)
        lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().pire_hip_run_lines_gather(self._h, raw.ctypes.data if raw.size else None, raw.size, delim, flags & ~FLAG_ON_DEVICE,
                                               _np_ptr(wm), _tail(delim if tail == -1 else tail), C.byref(lines),
                                               hits.ctypes.data if cap else None, cap, C.byref(cnt), text.ctypes.data if room else None,
                                               room, offsets.ctypes.data, C.byref(total), None))
        k = min(int(cnt.value), cap)
        return {"lines": int(lines.value), "hits": hits[:k], "count": int(cnt.value), "text": text[:min(int(total.value), room)],
                "offsets": offsets[:k + 1], "bytes": int(total.value)}

    def run_lines_gather_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int,
                                out_bytes_ptr: int, delim: int = 10, tail=-1, want_ptr=0, out_hits_ptr=0, hit_cap=0, out_text_ptr=0,
                                text_cap=0, out_offsets_ptr=0, stream: int = 0):
        """pire_hip_run_lines_gather on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
        _check(lib().pire_hip_run_lines_gather(self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, want_ptr or None,
                                               _tail(delim if tail == -1 else tail), out_line_count_ptr or None, out_hits_ptr or None,
                                               hit_cap, out_hit_count_ptr or None, out_text_ptr or None, text_cap,
                                               out_offsets_ptr or None, out_bytes_ptr or None, stream or None))

    # --- raw bytes in, the lines that match and their neighbours out (pire_hip_run_lines_context_select / _gather)
    def run_lines_context_host(self, raw, before: int = 0, after: int = 0, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, want=None,
                               gather=False, tail=-1, line_cap=None, text_cap=None):
        """pire_hip_run_lines_context_select (gather=True: _gather) on a host buffer: {"lines", "context" u64[k], "flags" u8[k],
        "spans" u64[k, 2], "count", "groups", "hits"} and, with gather, {"text", "offsets", "bytes"}.  tail -1 = the delimiter
        (grep -A -B --no-group-separator), None = none; line_cap None = room for every line."""
        raw = _raw_bytes(raw)
        wm = self.want_mask(want)
        front = [self._h, raw.ctypes.data if raw.size else None, raw.size, delim, flags & ~FLAG_ON_DEVICE, _np_ptr(wm)]
        return _lines_context_host(lib().pire_hip_run_lines_context_select, lib().pire_hip_run_lines_context_gather, front, raw, delim,
                                   before, after, tail, line_cap, text_cap, gather)

    def run_lines_context_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_sel_count_ptr: int, before: int = 0,
                                 after: int = 0, delim: int = 10, want_ptr=0, out_lines_ptr=0, out_line_flags_ptr=0,
                                 out_line_spans_ptr=0, line_cap=0, out_group_count_ptr=0, out_hit_count_ptr=0, out_bytes_ptr=None,
                                 tail=-1, out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
        """pire_hip_run_lines_context_select on device pointers -- out_bytes_ptr not None: _gather -- (synchronises `stream`
        once, as run_lines_select_device does)."""
        front = [self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, want_ptr or None]
        _lines_context_device(lib().pire_hip_run_lines_context_select, lib().pire_hip_run_lines_context_gather, front, before, after,
                              delim, tail, out_line_count_ptr, out_sel_count_ptr, out_lines_ptr, out_line_flags_ptr, out_line_spans_ptr,
                              line_cap, out_group_count_ptr, out_hit_count_ptr, out_bytes_ptr, out_text_ptr, text_cap, out_offsets_ptr,
                              stream)

    # --- the bytes of many files in, the matching lines by file out (pire_hip_run_lines_files_select)
    def run_lines_files_host(self, raw, file_bytes, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, want=None, without=False, hit_cap=None,
                             file_cap=None):
        """pire_hip_run_lines_files_select on a host buffer and file_bytes[files + 1]: {"lines", "hits" u64[k], "spans" u64[k, 2],
        "hit_file" u64[k], "hit_line" u64[k], "count", "file_lines" u64[files + 1], "first" u64[files + 1], "files" u64[m],
        "file_count", "straddles"}; hit_cap None = room for a hit on every line, file_cap None = room for every file."""
        raw = _raw_bytes(raw)
        wm = self.want_mask(want)
        front = [self._h, raw.ctypes.data if raw.size else None, raw.size, delim, flags & ~FLAG_ON_DEVICE, _np_ptr(wm)]
        return _lines_files_host(lib().pire_hip_run_lines_files_select, front, raw, file_bytes, without, hit_cap, file_cap)

    def run_lines_files_device(self, raw_ptr: int, size: int, flags, file_bytes_ptr: int, files: int, out_line_count_ptr: int,
                               out_hit_count_ptr: int, out_file_count_ptr: int, out_straddles_ptr: int, delim: int = 10, want_ptr=0,
                               without=False, out_hits_ptr=0, out_hit_spans_ptr=0, out_hit_file_ptr=0, out_hit_line_ptr=0, hit_cap=0,
                               out_file_lines_ptr=0, out_file_first_ptr=0, out_files_ptr=0, file_cap=0, stream: int = 0):
        """pire_hip_run_lines_files_select on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
        front = [self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, want_ptr or None]
        _lines_files_device(lib().pire_hip_run_lines_files_select, front, file_bytes_ptr, files, without, out_line_count_ptr, out_hits_ptr,
                            out_hit_spans_ptr, out_hit_file_ptr, out_hit_line_ptr, hit_cap, out_hit_count_ptr, out_file_lines_ptr,
                            out_file_first_ptr, out_files_ptr, file_cap, out_file_count_ptr, out_straddles_ptr, stream)

    # --- raw bytes in, the lines whose column matches out (pire_hip_run_lines_field_select / _gather): the results of the two
    # methods above, hits and spans being whole lines
    def run_lines_field_select_host(self, raw, field: int, sep: int = 9, delim: int = 10, rest: bool = False,
                                    flags=FLAG_BEGIN | FLAG_END, want=None, hit_cap=None, hit_masks=True):
        """pire_hip_run_lines_field_select on a host buffer: what run_lines_select_host returns, the scan on column `field`."""
        raw = _raw_bytes(raw)
        wm = self.want_mask(want)
        cap = raw.size if hit_cap is None else int(hit_cap)
        w = self.mask_words
        hits = np.zeros(cap, dtype=np.uint64)
        spans = np.zeros((cap, 2), dtype=np.uint64)
        masks = np.zeros((cap, w), dtype=np.uint64) if hit_masks else None
        lines, cnt = C.c_uint64(0), C.c_uint64(0)
        _check(lib().pire_hip_run_lines_field_select(self._h, raw.ctypes.data if raw.size else None, raw.size, delim, sep, field,
                                                     FIELDS_REST if rest else 0, flags & ~FLAG_ON_DEVICE, _np_ptr(wm), C.byref(lines),
                                                     hits.ctypes.data if cap else None, spans.ctypes.data if cap else None,
                                                     _np_ptr(masks) if cap else None, cap, C.byref(cnt), None))
        k = min(int(cnt.value), cap)
        return {"lines": int(lines.value), "hits": hits[:k], "spans": spans[:k], "hit_masks": None if masks is None else masks[:k],
                "count": int(cnt.value)}

    def run_lines_field_select_device(self, raw_ptr: int, size: int, field: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int,
                                      sep: int = 9, delim: int = 10, rest: bool = False, want_ptr=0, out_hits_ptr=0,
                                      out_hit_spans_ptr=0, out_hit_masks_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_run_lines_field_select on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
        _check(lib().pire_hip_run_lines_field_select(self._h, raw_ptr or None, size, delim, sep, field, FIELDS_REST if rest else 0,
                                                     flags | FLAG_ON_DEVICE, want_ptr or None, out_line_count_ptr or None,
                                                     out_hits_ptr or None, out_hit_spans_ptr or None, out_hit_masks_ptr or None,
                                                     hit_cap, out_hit_count_ptr or None, stream or None))

    def run_lines_field_gather_host(self, raw, field: int, sep: int = 9, delim: int = 10, rest: bool = False,
                                    flags=FLAG_BEGIN | FLAG_END, want=None, tail=-1, hit_cap=None, text_cap=None):
        """pire_hip_run_lines_field_gather on a host buffer: what run_lines_gather_host returns, the scan on column `field`."""
        raw = _raw_bytes(raw)
        wm = self.want_mask(want)
        cap = raw.size if hit_cap is None else int(hit_cap)
        room = raw.size + cap if text_cap is None else int(text_cap)
        hits = np.zeros(cap, dtype=np.uint64)
        text = np.zeros(max(room, 1), dtype=np.uint8)
        offsets = np.zeros(cap + 1, dtype=np.uint64)
        lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().pire_hip_run_lines_field_gather(self._h, raw.ctypes.data if raw.size else None, raw.size, delim, sep, field,
                                                     FIELDS_REST if rest else 0, flags & ~FLAG_ON_DEVICE, _np_ptr(wm),
                                                     _tail(delim if tail == -1 else tail), C.byref(lines),
                                                     hits.ctypes.data if cap else None, cap, C.byref(cnt),
                                                     text.ctypes.data if room else None, room, offsets.ctypes.data, C.byref(total), None))
        k = min(int(cnt.value), cap)
        return {"lines": int(lines.value), "hits": hits[:k], "count": int(cnt.value), "text": text[:min(int(total.value), room)],
                "offsets": offsets[:k + 1], "bytes": int(total.value)}

    def run_lines_field_gather_device(self, raw_ptr: int, size: int, field: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int,
                                      out_bytes_ptr: int, sep: int = 9, delim: int = 10, rest: bool = False, tail=-1, want_ptr=0,
                                      out_hits_ptr=0, hit_cap=0, out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
        """pire_hip_run_lines_field_gather on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
        _check(lib().pire_hip_run_lines_field_gather(self._h, raw_ptr or None, size, delim, sep, field, FIELDS_REST if rest else 0,
                                                     flags | FLAG_ON_DEVICE, want_ptr or None, _tail(delim if tail == -1 else tail),
                                                     out_line_count_ptr or None, out_hits_ptr or None, hit_cap,
                                                     out_hit_count_ptr or None, out_text_ptr or None, text_cap,
                                                     out_offsets_ptr or None, out_bytes_ptr or None, stream or None))

    def run_half_final(self, text, offsets, flags=FLAG_BEGIN | FLAG_END):
        """The table walked as a Pire::HalfFinalScanner: (StateIndex, Final, Result[n, regexps]) for host strings."""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        idx = np.empty(n, dtype=np.uint32)
        fin = np.empty(n, dtype=np.uint8)
        res = np.zeros((n, max(self.RegexpsCount, 1)), dtype=np.uint32)
        _check(lib().pire_hip_run_half_final(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                             flags & ~FLAG_ON_DEVICE, idx.ctypes.data, fin.ctypes.data,
                                             res.ctypes.data, None))
        return idx, fin, res[:, :self.RegexpsCount]

    def run_half_final_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_idx_ptr=0, out_final_ptr=0,
                              out_results_ptr=0, stream: int = 0):
        _check(lib().pire_hip_run_half_final(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                             out_idx_ptr or None, out_final_ptr or None, out_results_ptr or None,
                                             stream or None))

    # --- the strings that count (pire_hip_run_half_final_select, pire_hip_half_final_lines_select)
    def run_half_final_select(self, text, offsets, flags=FLAG_BEGIN | FLAG_END, min_count=None, all=False, hit_cap: Optional[int] = None,
                              results=True):
        """pire_hip_run_half_final_select on host strings: what count_select_host returns and, with results, {"idx", "final",
        "results"}; without, the library keeps the rows to itself."""
        text = _raw_bytes(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, regexps = len(offsets) - 1, self.RegexpsCount
        idx, fin = (np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint8)) if results else (None, None)
        res = np.zeros((n, max(regexps, 1)), dtype=np.uint32) if results else None
        out = _CountOut(regexps, n, hit_cap, True, True, True)
        _check(lib().pire_hip_run_half_final_select(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                                    flags & ~FLAG_ON_DEVICE, _np_ptr(idx), _np_ptr(fin), _np_ptr(res),
                                                    _np_ptr(_min_count(min_count, regexps)), COUNT_ALL if all else 0, *out.args(), None))
        got = out.result()
        if results:
            got.update(idx=idx, final=fin, results=res[:, :regexps])
        return got

    def run_half_final_select_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_hit_count_ptr: int, min_count_ptr=0,
                                     all=False, out_idx_ptr=0, out_final_ptr=0, out_results_ptr=0, out_totals_ptr=0, out_hits_ptr=0,
                                     out_hit_results_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_run_half_final_select on device pointers: only enqueues on `stream`."""
        _check(lib().pire_hip_run_half_final_select(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                                    out_idx_ptr or None, out_final_ptr or None, out_results_ptr or None,
                                                    min_count_ptr or None, COUNT_ALL if all else 0, out_totals_ptr or None,
                                                    out_hits_ptr or None, out_hit_results_ptr or None, hit_cap,
                                                    out_hit_count_ptr or None, stream or None))

    def half_final_lines_select_host(self, raw, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, min_count=None, all=False, hit_cap=None):
        """pire_hip_half_final_lines_select on a host buffer: what count_select_host returns and {"lines", "spans"}; hit_cap None =
        room for a hit on every line (no more lines than bytes)."""
        raw = _raw_bytes(raw)
        regexps = self.RegexpsCount
        out = _CountOut(regexps, raw.size, hit_cap, True, True, True)
        spans = np.zeros((out.cap, 2), dtype=np.uint64)
        lines = C.c_uint64(0)
        a = out.args()
        _check(lib().pire_hip_half_final_lines_select(self._h, raw.ctypes.data if raw.size else None, raw.size, delim,
                                                      flags & ~FLAG_ON_DEVICE, _np_ptr(_min_count(min_count, regexps)),
                                                      COUNT_ALL if all else 0, C.byref(lines), a[0], a[1],
                                                      spans.ctypes.data if out.cap else None, a[2], a[3], a[4], None))
        got = out.result()
        got.update(lines=int(lines.value), spans=spans[:len(got["hits"])])
        return got

    def half_final_lines_select_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int,
                                       delim: int = 10, min_count_ptr=0, all=False, out_totals_ptr=0, out_hits_ptr=0, out_hit_spans_ptr=0,
                                       out_hit_results_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_half_final_lines_select on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
        _check(lib().pire_hip_half_final_lines_select(self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, min_count_ptr or None,
                                                      COUNT_ALL if all else 0, out_line_count_ptr or None, out_totals_ptr or None,
                                                      out_hits_ptr or None, out_hit_spans_ptr or None, out_hit_results_ptr or None,
                                                      hit_cap, out_hit_count_ptr or None, stream or None))

    def run_half_final_device_host_offsets(self, text_ptr: int, offsets: np.ndarray, flags, out_idx_ptr=0,
                                           out_final_ptr=0, out_results_ptr=0, stream: int = 0):
        """Resident text, offsets on the host (PIRE_HIP_RUN_HOST_OFFSETS); outputs on the device."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _check(lib().pire_hip_run_half_final(self._h, text_ptr or None, offsets.ctypes.data, len(offsets) - 1,
                                             flags | FLAG_ON_DEVICE | FLAG_HOST_OFFSETS, out_idx_ptr or None,
                                             out_final_ptr or None, out_results_ptr or None, stream or None))

    def prefix(self, text, offsets, longest: bool, through_begin=False, through_end=False, generic=False):
        """LongestPrefix / ShortestPrefix lengths (-1 = no prefix) for host strings."""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.empty(n, dtype=np.int64)
        _check(lib().pire_hip_prefix(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                     int(longest), int(through_begin), int(through_end), FLAG_GENERIC if generic else 0,
                                     out.ctypes.data, None))
        return out

    def prefix_device(self, text_ptr: int, offsets_ptr: int, n: int, longest: bool, out_len_ptr: int,
                      through_begin=False, through_end=False, stream: int = 0, generic=False):
        _check(lib().pire_hip_prefix(self._h, text_ptr or None, offsets_ptr or None, n, int(longest), int(through_begin),
                                     int(through_end), FLAG_ON_DEVICE | (FLAG_GENERIC if generic else 0),
                                     out_len_ptr or None, stream or None))

    def suffix(self, text, offsets, longest: bool, through_end=False, through_begin=False):
        """LongestSuffix / ShortestSuffix lengths (-1 = the reference's null) for host strings, walked backwards."""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.empty(n, dtype=np.int64)
        _check(lib().pire_hip_suffix(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                     int(longest), int(through_end), int(through_begin), 0, out.ctypes.data, None))
        return out

    def suffix_device(self, text_ptr: int, offsets_ptr: int, n: int, longest: bool, out_len_ptr: int,
                      through_end=False, through_begin=False, stream: int = 0):
        _check(lib().pire_hip_suffix(self._h, text_ptr or None, offsets_ptr or None, n, int(longest), int(through_end),
                                     int(through_begin), FLAG_ON_DEVICE, out_len_ptr or None, stream or None))

    def check_failures(self) -> int:
        """Failures counted by the checked kernel build (PIRE_HIP_CHECKED=1) since the last call."""
        v = C.c_uint64(0)
        _check(lib().pire_hip_table_check_failures(self._h, C.byref(v)))
        return int(v.value)

    def step_device(self, state_ptr: int, n: int, ch: int, stream: int = 0):
        _check(lib().pire_hip_step(self._h, state_ptr, n, ch, stream or None))


class SlowTable:
    """An ingested Pire::SlowScanner (from SlowScanner::Save() bytes)."""

    def __init__(self, blob: bytes):
        L = lib()
        h = C.c_void_p()
        blob = bytes(blob)
        _check(L.pire_hip_slow_table_create(blob, len(blob), C.byref(h)))
        self._h = h
        self.info = SlowInfo()
        _check(L.pire_hip_slow_table_get_info(h, C.byref(self.info)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            try:
                _lib.pire_hip_slow_table_destroy(h)
            except Exception:
                pass
            self._h = None

    Size = property(lambda s: s.info.states)
    LettersCount = property(lambda s: s.info.letters)
    Empty = property(lambda s: bool(s.info.empty))
    words = property(lambda s: s.info.words)

    PLAN_KERNELS = ("slow_list", "slow", "slow_wide")   # as last_kernel() names them

    def plan(self, n: int, ragged: bool = True, cus: int = 0) -> dict:
        """What a run of n strings would launch under the current configuration (pire_hip_slow_table_plan); cus = 0: the
        current device's compute units, any other value needs no device."""
        out = (C.c_uint32 * 24)()
        _check(lib().pire_hip_slow_table_plan(self._h, n, int(bool(ragged)), cus, C.byref(out)))
        grid = lambda i: {"threads": out[i], "blocks": out[i + 1], "lds_bytes": out[i + 2], "passes": out[i + 3]}
        return {"kernel": self.PLAN_KERNELS[out[0]], "walker": self.PLAN_KERNELS[out[1]], "k": out[2],
                "list_table": bool(out[3]), "single_in_lds": bool(out[4]), "masks_in_lds": bool(out[5]), **grid(6),
                "waves": out[10], "pos_in_lds": bool(out[11]), "jumps_in_lds": bool(out[12]), "sets_in_lds": bool(out[13]),
                "by_length": bool(out[14]), "walk": grid(15), "cus": out[19]}

    def run(self, text, offsets, flags=FLAG_BEGIN | FLAG_END, counts=False):
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        fin = np.empty(n, dtype=np.uint8)
        bits = np.empty((n, self.words), dtype=np.uint32)
        cnt = np.zeros(2, dtype=np.uint64) if counts else None
        _check(lib().pire_hip_slow_run(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                       flags & ~FLAG_ON_DEVICE, fin.ctypes.data, bits.ctypes.data, _np_ptr(cnt), None))
        return (fin, bits, cnt) if counts else (fin, bits)

    def run_strings(self, strings, **kw):
        offs = np.zeros(len(strings) + 1, dtype=np.uint64)
        if strings:
            offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        return self.run(np.frombuffer(b"".join(strings), dtype=np.uint8), offs, **kw)

    def run_device(self, text_ptr, offsets_ptr, n, flags, out_final_ptr=0, out_bits_ptr=0, out_counts_ptr=0, stream=0):
        """pire_hip_slow_run with every pointer on the device (offsets: n + 1 uint64)."""
        _check(lib().pire_hip_slow_run(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                       out_final_ptr or None, out_bits_ptr or None, out_counts_ptr or None, stream or None))

    def run_strided_device(self, text_ptr, n, length, stride, flags, out_final_ptr=0, out_bits_ptr=0, out_counts_ptr=0,
                           stream=0):
        _check(lib().pire_hip_slow_run_strided(self._h, text_ptr or None, n, length, stride, flags | FLAG_ON_DEVICE,
                                               out_final_ptr or None, out_bits_ptr or None, out_counts_ptr or None,
                                               stream or None))

    # --- the scan and the hit list behind one call (pire_hip_slow_run_select); invert: the strings that did NOT match
    def run_select(self, text, offsets, flags=FLAG_BEGIN | FLAG_END, invert=False, hit_cap: Optional[int] = None, results=True):
        """pire_hip_slow_run_select on host strings: what final_select_host returns and, with results, {"final", "bits"};
        without, the library keeps the flags to itself."""
        text = _raw_bytes(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        fin = np.empty(n, dtype=np.uint8) if results else None
        bits = np.empty((n, self.words), dtype=np.uint32) if results else None
        cap = n if hit_cap is None else int(hit_cap)
        hits = np.zeros(cap, dtype=np.uint64)
        cnt = C.c_uint64(0)
        _check(lib().pire_hip_slow_run_select(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                              flags & ~FLAG_ON_DEVICE, _final_mode(invert), _np_ptr(fin), _np_ptr(bits), None,
                                              hits.ctypes.data if cap else None, cap, C.byref(cnt), None))
        got = {"hits": hits[:min(int(cnt.value), cap)], "count": int(cnt.value)}
        if results:
            got.update(final=fin, bits=bits)
        return got

    def run_select_strings(self, strings, **kw):
        offs = np.zeros(len(strings) + 1, dtype=np.uint64)
        if strings:
            offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        return self.run_select(np.frombuffer(b"".join(strings), dtype=np.uint8), offs, **kw)

    def run_select_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_hit_count_ptr: int, invert=False, out_final_ptr=0,
                          out_bits_ptr=0, out_counts_ptr=0, out_hits_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_slow_run_select on device pointers: only enqueues on `stream`."""
        _check(lib().pire_hip_slow_run_select(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE, _final_mode(invert),
                                              out_final_ptr or None, out_bits_ptr or None, out_counts_ptr or None, out_hits_ptr or None,
                                              hit_cap, out_hit_count_ptr or None, stream or None))

    def run_select_strided_device(self, text_ptr: int, n: int, length: int, stride: int, flags, out_hit_count_ptr: int, invert=False,
                                  out_final_ptr=0, out_bits_ptr=0, out_counts_ptr=0, out_hits_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_slow_run_select_strided on device pointers: only enqueues on `stream`."""
        _check(lib().pire_hip_slow_run_select_strided(self._h, text_ptr or None, n, length, stride, flags | FLAG_ON_DEVICE,
                                                      _final_mode(invert), out_final_ptr or None, out_bits_ptr or None,
                                                      out_counts_ptr or None, out_hits_ptr or None, hit_cap, out_hit_count_ptr or None,
                                                      stream or None))

    # --- raw bytes in, the lines that match (or, inverted, do not) out (pire_hip_slow_lines_select / _gather)
    def lines_select_host(self, raw, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, invert=False, hit_cap=None):
        """pire_hip_slow_lines_select on a host buffer: {"lines", "hits", "spans", "count"}; hit_cap None = room for a hit on
        every line (no more lines than bytes)."""
        raw = _raw_bytes(raw)
        cap = raw.size if hit_cap is None else int(hit_cap)
        hits = np.zeros(cap, dtype=np.uint64)
        spans = np.zeros((cap, 2), dtype=np.uint64)
        lines, cnt = C.c_uint64(0), C.c_uint64(0)
        _check(lib().pire_hip_slow_lines_select(self._h, raw.ctypes.data if raw.size else None, raw.size, delim, flags & ~FLAG_ON_DEVICE,
                                                _final_mode(invert), C.byref(lines), hits.ctypes.data if cap else None,
                                                spans.ctypes.data if cap else None, cap, C.byref(cnt), None))
        k = min(int(cnt.value), cap)
        return {"lines": int(lines.value), "hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}

    def lines_select_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int, delim: int = 10,
                            invert=False, out_hits_ptr=0, out_hit_spans_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_slow_lines_select on device pointers (synchronises `stream` once, as Table.run_lines_select_device does)."""
        _check(lib().pire_hip_slow_lines_select(self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, _final_mode(invert),
                                                out_line_count_ptr or None, out_hits_ptr or None, out_hit_spans_ptr or None, hit_cap,
                                                out_hit_count_ptr or None, stream or None))

    def lines_gather_host(self, raw, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, invert=False, tail=-1, hit_cap=None, text_cap=None):
        """pire_hip_slow_lines_gather on a host buffer: {"lines", "hits", "count", "text", "offsets", "bytes"}.  tail -1 = the
        delimiter (grep's output; inverted: grep -v's), None = none; hit_cap None = room for a hit on every line, text_cap None =
        for all of them."""
        raw = _raw_bytes(raw)
        cap = raw.size if hit_cap is None else int(hit_cap)
        room = raw.size + cap if text_cap is None else int(text_cap)
        hits = np.zeros(cap, dtype=np.uint64)
        text = np.zeros(max(room, 1), dtype=np.uint8)
        offsets = np.zeros(cap + 1, dtype=np.uint64)
        lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().pire_hip_slow_lines_gather(self._h, raw.ctypes.data if raw.size else None, raw.size, delim, flags & ~FLAG_ON_DEVICE,
                                                _final_mode(invert), _tail(delim if tail == -1 else tail), C.byref(lines),
                                                hits.ctypes.data if cap else None, cap, C.byref(cnt), text.ctypes.data if room else None,
                                                room, offsets.ctypes.data, C.byref(total), None))
        k = min(int(cnt.value), cap)
        return {"lines": int(lines.value), "hits": hits[:k], "count": int(cnt.value), "text": text[:min(int(total.value), room)],
                "offsets": offsets[:k + 1], "bytes": int(total.value)}

    def lines_gather_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int, out_bytes_ptr: int,
                            delim: int = 10, invert=False, tail=-1, out_hits_ptr=0, hit_cap=0, out_text_ptr=0, text_cap=0,
                            out_offsets_ptr=0, stream: int = 0):
        """pire_hip_slow_lines_gather on device pointers (synchronises `stream` once, as Table.run_lines_select_device does)."""
        _check(lib().pire_hip_slow_lines_gather(self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, _final_mode(invert),
                                                _tail(delim if tail == -1 else tail), out_line_count_ptr or None, out_hits_ptr or None,
                                                hit_cap, out_hit_count_ptr or None, out_text_ptr or None, text_cap,
                                                out_offsets_ptr or None, out_bytes_ptr or None, stream or None))

    # --- raw bytes in, the lines that match (or, inverted, do not) and their neighbours out (pire_hip_slow_lines_context_*)
    def lines_context_host(self, raw, before: int = 0, after: int = 0, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, invert=False,
                           gather=False, tail=-1, line_cap=None, text_cap=None):
        """pire_hip_slow_lines_context_select (gather=True: _gather) on a host buffer: what Table.run_lines_context_host returns;
        invert: grep -v -C."""
        raw = _raw_bytes(raw)
        front = [self._h, raw.ctypes.data if raw.size else None, raw.size, delim, flags & ~FLAG_ON_DEVICE, _final_mode(invert)]
        return _lines_context_host(lib().pire_hip_slow_lines_context_select, lib().pire_hip_slow_lines_context_gather, front, raw, delim,
                                   before, after, tail, line_cap, text_cap, gather)

    def lines_context_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_sel_count_ptr: int, before: int = 0,
                             after: int = 0, delim: int = 10, invert=False, out_lines_ptr=0, out_line_flags_ptr=0, out_line_spans_ptr=0,
                             line_cap=0, out_group_count_ptr=0, out_hit_count_ptr=0, out_bytes_ptr=None, tail=-1, out_text_ptr=0,
                             text_cap=0, out_offsets_ptr=0, stream: int = 0):
        """pire_hip_slow_lines_context_select on device pointers -- out_bytes_ptr not None: _gather -- (synchronises `stream`
        once, as Table.run_lines_select_device does)."""
        front = [self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, _final_mode(invert)]
        _lines_context_device(lib().pire_hip_slow_lines_context_select, lib().pire_hip_slow_lines_context_gather, front, before, after,
                              delim, tail, out_line_count_ptr, out_sel_count_ptr, out_lines_ptr, out_line_flags_ptr, out_line_spans_ptr,
                              line_cap, out_group_count_ptr, out_hit_count_ptr, out_bytes_ptr, out_text_ptr, text_cap, out_offsets_ptr,
                              stream)

    # --- the bytes of many files in, the lines that match (or, inverted, do not) by file out (pire_hip_slow_lines_files_select)
    def lines_files_host(self, raw, file_bytes, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, invert=False, without=False, hit_cap=None,
                         file_cap=None):
        """pire_hip_slow_lines_files_select on a host buffer: what Table.run_lines_files_host returns; invert: grep -v -c / -l."""
        raw = _raw_bytes(raw)
        front = [self._h, raw.ctypes.data if raw.size else None, raw.size, delim, flags & ~FLAG_ON_DEVICE, _final_mode(invert)]
        return _lines_files_host(lib().pire_hip_slow_lines_files_select, front, raw, file_bytes, without, hit_cap, file_cap)

    def lines_files_device(self, raw_ptr: int, size: int, flags, file_bytes_ptr: int, files: int, out_line_count_ptr: int,
                           out_hit_count_ptr: int, out_file_count_ptr: int, out_straddles_ptr: int, delim: int = 10, invert=False,
                           without=False, out_hits_ptr=0, out_hit_spans_ptr=0, out_hit_file_ptr=0, out_hit_line_ptr=0, hit_cap=0,
                           out_file_lines_ptr=0, out_file_first_ptr=0, out_files_ptr=0, file_cap=0, stream: int = 0):
        """pire_hip_slow_lines_files_select on device pointers (synchronises `stream` once, as Table.run_lines_select_device does)."""
        front = [self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, _final_mode(invert)]
        _lines_files_device(lib().pire_hip_slow_lines_files_select, front, file_bytes_ptr, files, without, out_line_count_ptr, out_hits_ptr,
                            out_hit_spans_ptr, out_hit_file_ptr, out_hit_line_ptr, hit_cap, out_hit_count_ptr, out_file_lines_ptr,
                            out_file_first_ptr, out_files_ptr, file_cap, out_file_count_ptr, out_straddles_ptr, stream)


class SlowCaptureTable:
    """An ingested Pire::SlowCapturingScanner (from its Save() bytes, which carry the actions): exact captures, greedy and lazy."""

    def __init__(self, blob: bytes):
        L = lib()
        h = C.c_void_p()
        blob = bytes(blob)
        _check(L.pire_hip_slow_capture_table_create(blob, len(blob), C.byref(h)))
        self._h = h
        self.info = SlowCaptureInfo()
        _check(L.pire_hip_slow_capture_table_get_info(h, C.byref(self.info)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            try:
                _lib.pire_hip_slow_capture_table_destroy(h)
            except Exception:
                pass
            self._h = None

    Size = property(lambda s: s.info.states)
    LettersCount = property(lambda s: s.info.letters)
    Empty = property(lambda s: bool(s.info.empty))

    def image(self) -> dict:
        """pire_hip_slow_capture_table_image: {"list_pos", "entries", "state_flags", "init" [init_len][3], "init_match" (or None),
        "letters" [260]} -- the flat form of the reference's walk."""
        i = self.info
        pos = np.zeros(i.states * i.letters + 1, dtype=np.uint32)
        entries = np.zeros(max(i.entries, 1), dtype=np.uint32)
        flags = np.zeros(i.states, dtype=np.uint8)
        init = np.zeros((max(i.init_len, 1), 3), dtype=np.int64)
        match = np.zeros(3, dtype=np.int64)
        letters = np.zeros(260, dtype=np.uint8)
        _check(lib().pire_hip_slow_capture_table_image(self._h, pos.ctypes.data, entries.ctypes.data, entries.size, flags.ctypes.data,
                                                       init.ctypes.data, match.ctypes.data, letters.ctypes.data))
        return {"list_pos": pos, "entries": entries[:i.entries], "state_flags": flags, "init": init[:i.init_len],
                "init_match": match if i.init_matched else None, "letters": letters}

    def run(self, text, offsets, flags=0):
        """pire_hip_slow_capture_run on host strings: (captured, begin, end, matched)"""
        text = _raw_bytes(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        cap, mat = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        b, e = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        _check(lib().pire_hip_slow_capture_run(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                               flags & ~FLAG_ON_DEVICE, cap.ctypes.data, b.ctypes.data, e.ctypes.data, mat.ctypes.data, None))
        return cap, b, e, mat

    def run_strings(self, strings, **kw):
        offs = np.zeros(len(strings) + 1, dtype=np.uint64)
        if strings:
            offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        return self.run(np.frombuffer(b"".join(strings), dtype=np.uint8), offs, **kw)

    def run_device(self, text_ptr, offsets_ptr, n, out_captured_ptr, out_begin_ptr, out_end_ptr, out_matched_ptr=0, flags=0, stream=0):
        """pire_hip_slow_capture_run with every pointer on the device (offsets: n + 1 uint64): only enqueues on `stream`."""
        _check(lib().pire_hip_slow_capture_run(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                               out_captured_ptr or None, out_begin_ptr or None, out_end_ptr or None,
                                               out_matched_ptr or None, stream or None))

    def run_select(self, text, offsets, hit_cap: Optional[int] = None, positions=True, lists=True, flags=0):
        """pire_hip_slow_capture_run_select on host strings: {"hits", "spans", "count"} and, with positions, {"captured", "begin",
        "end", "matched"}; without, the library keeps those arrays to itself.  hit_cap None = room for every string."""
        text = _raw_bytes(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        cap = (n if hit_cap is None else int(hit_cap)) if lists else 0
        c, m = (np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)) if positions else (None, None)
        b, e = (np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)) if positions else (None, None)
        hits = np.zeros(cap, dtype=np.uint64)
        spans = np.zeros((cap, 2), dtype=np.uint64)
        cnt = C.c_uint64(0)
        _check(lib().pire_hip_slow_capture_run_select(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                                      flags & ~FLAG_ON_DEVICE, _np_ptr(c), _np_ptr(b), _np_ptr(e), _np_ptr(m),
                                                      hits.ctypes.data if cap else None, spans.ctypes.data if cap else None, cap,
                                                      C.byref(cnt), None))
        k = min(int(cnt.value), cap)
        out = {"hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}
        if positions:
            out.update(captured=c, begin=b, end=e, matched=m)
        return out

    def run_select_device(self, text_ptr: int, offsets_ptr: int, n: int, out_hit_count_ptr: int, out_captured_ptr=0, out_begin_ptr=0,
                          out_end_ptr=0, out_matched_ptr=0, out_hits_ptr=0, out_spans_ptr=0, hit_cap=0, flags=0, stream: int = 0):
        """pire_hip_slow_capture_run_select on device pointers: only enqueues on `stream`."""
        _check(lib().pire_hip_slow_capture_run_select(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                                      out_captured_ptr or None, out_begin_ptr or None, out_end_ptr or None,
                                                      out_matched_ptr or None, out_hits_ptr or None, out_spans_ptr or None, hit_cap,
                                                      out_hit_count_ptr or None, stream or None))

    def lines_gather_host(self, raw, delim: int = 10, tail=-1, hit_cap=None, text_cap=None, gather=True, flags=0):
        """pire_hip_slow_capture_lines_gather on a host buffer: {"lines", "hits", "spans", "count"} and, with gather, {"text",
        "offsets", "bytes"}.  tail -1 = the delimiter, None = none; hit_cap None = room for a hit on every line, text_cap None
        = for all of them."""
        raw = _raw_bytes(raw)
        cap = raw.size if hit_cap is None else int(hit_cap)
        room = (raw.size + cap if text_cap is None else int(text_cap)) if gather else 0
        hits = np.zeros(cap, dtype=np.uint64)
        spans = np.zeros((cap, 2), dtype=np.uint64)
        text = np.zeros(max(room, 1), dtype=np.uint8)
        offsets = np.zeros(cap + 1, dtype=np.uint64)
        lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().pire_hip_slow_capture_lines_gather(self._h, raw.ctypes.data if raw.size else None, raw.size, delim,
                                                        flags & ~FLAG_ON_DEVICE, _tail(delim if tail == -1 else tail), C.byref(lines),
                                                        hits.ctypes.data if cap else None, spans.ctypes.data if cap else None, cap,
                                                        C.byref(cnt), text.ctypes.data if room else None, room,
                                                        offsets.ctypes.data if gather else None, C.byref(total) if gather else None, None))
        k = min(int(cnt.value), cap)
        out = {"lines": int(lines.value), "hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}
        if gather:
            out.update(text=text[:min(int(total.value), room)], offsets=offsets[:k + 1], bytes=int(total.value))
        return out

    def lines_gather_device(self, raw_ptr: int, size: int, out_line_count_ptr: int, out_hit_count_ptr: int, out_bytes_ptr=0,
                            delim: int = 10, tail=-1, out_hits_ptr=0, out_spans_ptr=0, hit_cap=0, out_text_ptr=0, text_cap=0,
                            out_offsets_ptr=0, flags=0, stream: int = 0):
        """pire_hip_slow_capture_lines_gather on device pointers (synchronises `stream` once, as Table.run_lines_select_device does)."""
        _check(lib().pire_hip_slow_capture_lines_gather(self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE,
                                                        _tail(delim if tail == -1 else tail), out_line_count_ptr or None,
                                                        out_hits_ptr or None, out_spans_ptr or None, hit_cap, out_hit_count_ptr or None,
                                                        out_text_ptr or None, text_cap, out_offsets_ptr or None, out_bytes_ptr or None,
                                                        stream or None))


class CountingTable:
    """An ingested Pire::CountingScanner / AdvancedCountingScanner (LoadedScanner::Save() bytes)."""

    BASIC, ADVANCED = 0, 1

    def __init__(self, blob: bytes, kind: int):
        L = lib()
        h = C.c_void_p()
        blob = bytes(blob)
        _check(L.pire_hip_counting_table_create(blob, len(blob), C.byref(h)))
        self._h = h
        self.kind = kind
        self.info = CountingInfo()
        _check(L.pire_hip_counting_table_get_info(h, C.byref(self.info)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            try:
                _lib.pire_hip_counting_table_destroy(h)
            except Exception:
                pass
            self._h = None

    Size = property(lambda s: s.info.states)
    LettersCount = property(lambda s: s.info.letters)
    RegexpsCount = property(lambda s: s.info.regexps)
    initial = property(lambda s: s.info.initial)

    def forms(self) -> dict:
        """Which device forms the table has (pire_hip_counting_table_forms)."""
        out = (C.c_uint32 * 8)()
        _check(lib().pire_hip_counting_table_forms(self._h, C.byref(out)))
        return {"packed_nreg": out[0], "packed_lds": out[1], "byte_rows": bool(out[2]), "byte_rows_lds": out[3],
                "letter_rows_nreg": out[4], "letter_rows_lds": out[5], "letter_rows_actions": out[6]}

    def run(self, text, offsets, flags=FLAG_BEGIN | FLAG_END):
        """(StateIndex[n], Result[n, regexps]) for host strings."""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        idx = np.empty(n, dtype=np.uint32)
        res = np.zeros((n, max(self.RegexpsCount, 1)), dtype=np.uint32)
        _check(lib().pire_hip_counting_run(self._h, self.kind, text.ctypes.data if text.size else None,
                                           offsets.ctypes.data, n, flags & ~FLAG_ON_DEVICE, idx.ctypes.data,
                                           res.ctypes.data, None))
        return idx, res[:, :self.RegexpsCount]

    def run_strings(self, strings, **kw):
        offs = np.zeros(len(strings) + 1, dtype=np.uint64)
        if strings:
            offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        return self.run(np.frombuffer(b"".join(strings), dtype=np.uint8), offs, **kw)

    def capture(self, text, offsets, flags=FLAG_BEGIN | FLAG_END):
        """The table walked as a Pire::CapturingScanner: (StateIndex, Final, captured, begin, end) for host strings."""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        idx = np.empty(n, dtype=np.uint32)
        fin = np.empty(n, dtype=np.uint8)
        b = np.empty(n, dtype=np.int64)
        e = np.empty(n, dtype=np.int64)
        _check(lib().pire_hip_capture_run(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                          flags & ~FLAG_ON_DEVICE, idx.ctypes.data, fin.ctypes.data, b.ctypes.data,
                                          e.ctypes.data, None))
        return idx, fin, ((b >= 0) & (e >= 0)).astype(np.uint8), b, e

    def capture_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_idx_ptr=0, out_final_ptr=0,
                       out_begin_ptr=0, out_end_ptr=0, stream: int = 0):
        _check(lib().pire_hip_capture_run(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                          out_idx_ptr or None, out_final_ptr or None, out_begin_ptr or None,
                                          out_end_ptr or None, stream or None))

    # --- the captured substrings as byte ranges (pire_hip_capture_run_select, pire_hip_capture_lines_gather)
    def capture_select(self, text, offsets, flags=FLAG_BEGIN | FLAG_END, need_final=False, hit_cap: Optional[int] = None,
                       positions=True):
        """pire_hip_capture_run_select on host strings: {"hits", "spans", "count"} and, with positions, {"idx", "final",
        "begin", "end"}; without, the library keeps those arrays to itself.  hit_cap None = room for every string."""
        text = _raw_bytes(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        cap = n if hit_cap is None else int(hit_cap)
        idx, fin = (np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint8)) if positions else (None, None)
        b, e = (np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)) if positions else (None, None)
        hits = np.zeros(cap, dtype=np.uint64)
        spans = np.zeros((cap, 2), dtype=np.uint64)
        cnt = C.c_uint64(0)
        _check(lib().pire_hip_capture_run_select(self._h, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                                 flags & ~FLAG_ON_DEVICE, int(bool(need_final)), _np_ptr(idx), _np_ptr(fin), _np_ptr(b),
                                                 _np_ptr(e), hits.ctypes.data if cap else None, spans.ctypes.data if cap else None, cap,
                                                 C.byref(cnt), None))
        k = min(int(cnt.value), cap)
        out = {"hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}
        if positions:
            out.update(idx=idx, final=fin, begin=b, end=e)
        return out

    def capture_select_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_hit_count_ptr: int, need_final=False,
                              out_idx_ptr=0, out_final_ptr=0, out_begin_ptr=0, out_end_ptr=0, out_hits_ptr=0, out_spans_ptr=0,
                              hit_cap=0, stream: int = 0):
        """pire_hip_capture_run_select on device pointers: only enqueues on `stream`."""
        _check(lib().pire_hip_capture_run_select(self._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                                 int(bool(need_final)), out_idx_ptr or None, out_final_ptr or None,
                                                 out_begin_ptr or None, out_end_ptr or None, out_hits_ptr or None,
                                                 out_spans_ptr or None, hit_cap, out_hit_count_ptr or None, stream or None))

    def capture_lines_gather_host(self, raw, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, need_final=False, tail=-1,
                                  hit_cap=None, text_cap=None, gather=True):
        """pire_hip_capture_lines_gather on a host buffer: {"lines", "hits", "spans", "count"} and, with gather, {"text",
        "offsets", "bytes"}.  tail -1 = the delimiter, None = none; hit_cap None = room for a hit on every line, text_cap None
        = for all of them."""
        raw = _raw_bytes(raw)
        cap = raw.size if hit_cap is None else int(hit_cap)
        room = (raw.size + cap if text_cap is None else int(text_cap)) if gather else 0
        hits = np.zeros(cap, dtype=np.uint64)
        spans = np.zeros((cap, 2), dtype=np.uint64)
        text = np.zeros(max(room, 1), dtype=np.uint8)
        offsets = np.zeros(cap + 1, dtype=np.uint64)
        lines, cnt, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().pire_hip_capture_lines_gather(self._h, raw.ctypes.data if raw.size else None, raw.size, delim,
                                                   flags & ~FLAG_ON_DEVICE, int(bool(need_final)), _tail(delim if tail == -1 else tail),
                                                   C.byref(lines), hits.ctypes.data if cap else None, spans.ctypes.data if cap else None,
                                                   cap, C.byref(cnt), text.ctypes.data if room else None, room,
                                                   offsets.ctypes.data if gather else None, C.byref(total) if gather else None, None))
        k = min(int(cnt.value), cap)
        out = {"lines": int(lines.value), "hits": hits[:k], "spans": spans[:k], "count": int(cnt.value)}
        if gather:
            out.update(text=text[:min(int(total.value), room)], offsets=offsets[:k + 1], bytes=int(total.value))
        return out

    def capture_lines_gather_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int,
                                    out_bytes_ptr=0, delim: int = 10, need_final=False, tail=-1, out_hits_ptr=0, out_spans_ptr=0,
                                    hit_cap=0, out_text_ptr=0, text_cap=0, out_offsets_ptr=0, stream: int = 0):
        """pire_hip_capture_lines_gather on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
        _check(lib().pire_hip_capture_lines_gather(self._h, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE,
                                                   int(bool(need_final)), _tail(delim if tail == -1 else tail),
                                                   out_line_count_ptr or None, out_hits_ptr or None, out_spans_ptr or None, hit_cap,
                                                   out_hit_count_ptr or None, out_text_ptr or None, text_cap,
                                                   out_offsets_ptr or None, out_bytes_ptr or None, stream or None))

    # --- the strings that count (pire_hip_counting_run_select, pire_hip_counting_lines_select)
    def run_select(self, text, offsets, flags=FLAG_BEGIN | FLAG_END, min_count=None, all=False, hit_cap: Optional[int] = None,
                              results=True):
        """pire_hip_counting_run_select on host strings: what count_select_host returns and, with results, {"idx", "results"}; without, the library keeps the rows to itself."""
        text = _raw_bytes(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, regexps = len(offsets) - 1, self.RegexpsCount
        idx = np.empty(n, dtype=np.uint32) if results else None
        res = np.zeros((n, max(regexps, 1)), dtype=np.uint32) if results else None
        out = _CountOut(regexps, n, hit_cap, True, True, True)
        _check(lib().pire_hip_counting_run_select(self._h, self.kind, text.ctypes.data if text.size else None, offsets.ctypes.data, n,
                                                    flags & ~FLAG_ON_DEVICE, _np_ptr(idx), _np_ptr(res),
                                                    _np_ptr(_min_count(min_count, regexps)), COUNT_ALL if all else 0, *out.args(), None))
        got = out.result()
        if results:
            got.update(idx=idx, results=res[:, :regexps])
        return got

    def run_select_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_hit_count_ptr: int, min_count_ptr=0,
                                     all=False, out_idx_ptr=0, out_results_ptr=0, out_totals_ptr=0, out_hits_ptr=0,
                                     out_hit_results_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_counting_run_select on device pointers: only enqueues on `stream`."""
        _check(lib().pire_hip_counting_run_select(self._h, self.kind, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                                    out_idx_ptr or None, out_results_ptr or None,
                                                    min_count_ptr or None, COUNT_ALL if all else 0, out_totals_ptr or None,
                                                    out_hits_ptr or None, out_hit_results_ptr or None, hit_cap,
                                                    out_hit_count_ptr or None, stream or None))

    def lines_select_host(self, raw, delim: int = 10, flags=FLAG_BEGIN | FLAG_END, min_count=None, all=False, hit_cap=None):
        """pire_hip_counting_lines_select on a host buffer: what count_select_host returns and {"lines", "spans"}; hit_cap None =
        room for a hit on every line (no more lines than bytes)."""
        raw = _raw_bytes(raw)
        regexps = self.RegexpsCount
        out = _CountOut(regexps, raw.size, hit_cap, True, True, True)
        spans = np.zeros((out.cap, 2), dtype=np.uint64)
        lines = C.c_uint64(0)
        a = out.args()
        _check(lib().pire_hip_counting_lines_select(self._h, self.kind, raw.ctypes.data if raw.size else None, raw.size, delim,
                                                      flags & ~FLAG_ON_DEVICE, _np_ptr(_min_count(min_count, regexps)),
                                                      COUNT_ALL if all else 0, C.byref(lines), a[0], a[1],
                                                      spans.ctypes.data if out.cap else None, a[2], a[3], a[4], None))
        got = out.result()
        got.update(lines=int(lines.value), spans=spans[:len(got["hits"])])
        return got

    def lines_select_device(self, raw_ptr: int, size: int, flags, out_line_count_ptr: int, out_hit_count_ptr: int,
                                       delim: int = 10, min_count_ptr=0, all=False, out_totals_ptr=0, out_hits_ptr=0, out_hit_spans_ptr=0,
                                       out_hit_results_ptr=0, hit_cap=0, stream: int = 0):
        """pire_hip_counting_lines_select on device pointers (synchronises `stream` once, as run_lines_select_device does)."""
        _check(lib().pire_hip_counting_lines_select(self._h, self.kind, raw_ptr or None, size, delim, flags | FLAG_ON_DEVICE, min_count_ptr or None,
                                                      COUNT_ALL if all else 0, out_line_count_ptr or None, out_totals_ptr or None,
                                                      out_hits_ptr or None, out_hit_spans_ptr or None, out_hit_results_ptr or None,
                                                      hit_cap, out_hit_count_ptr or None, stream or None))

    def run_device(self, text_ptr: int, offsets_ptr: int, n: int, flags, out_idx_ptr=0, out_results_ptr=0, stream: int = 0):
        _check(lib().pire_hip_counting_run(self._h, self.kind, text_ptr or None, offsets_ptr or None, n,
                                           flags | FLAG_ON_DEVICE, out_idx_ptr or None, out_results_ptr or None,
                                           stream or None))


class BatchRunner:
    """Batched twin of Pire::Runner / RunHelper (run.h:365-392):  BatchRunner(t).Begin().Run(text, offs).End()."""

    def __init__(self, table: Table, init_idx=None):
        self.table = table
        self._flags = 0
        self._init = init_idx
        self._text = None
        self._offsets = None
        self._result = None

    def Begin(self):
        self._flags |= FLAG_BEGIN
        return self

    def Run(self, text, offsets):
        self._text, self._offsets = text, offsets
        return self

    def End(self):
        self._flags |= FLAG_END
        return self

    def _go(self):
        if self._result is None:
            if self._text is None:
                raise ValueError("Run() was not called")
            self._result = self.table.run(self._text, self._offsets, flags=self._flags, init_idx=self._init)
        return self._result

    def State(self):
        """StateIndex of every string's end state (run.h:378)."""
        return self._go()[0]

    def Final(self):
        """operator bool of RunHelper, per string (run.h:380)."""
        return self._go()[1].astype(bool)


class Shard(C.Structure):
    """pire_hip_shard (include/pire_hip.h)."""
    _fields_ = [("text", C.c_void_p), ("n", C.c_uint64), ("len", C.c_uint64), ("stride", C.c_uint64),
                ("init_state_idx", C.c_void_p), ("out_state_idx", C.c_void_p), ("out_final", C.c_void_p)]


class ShardOffsets(C.Structure):
    """pire_hip_shard_offsets: one device's part of an offset batch (device pointers of that device)."""
    _fields_ = [("text", C.c_void_p), ("offsets", C.c_void_p), ("n", C.c_uint64), ("init_state_idx", C.c_void_p),
                ("out_state_idx", C.c_void_p), ("out_final", C.c_void_p)]


class MultiRunner:
    """pire_hip_multi: one process, several GPUs, strings sharded by index, match counters reduced over RCCL."""

    def __init__(self, devices=None, ndev: int = 0):
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            _check(lib().pire_hip_multi_create(arr, len(devices), C.byref(h)))
        else:
            _check(lib().pire_hip_multi_create(None, ndev, C.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.pire_hip_multi_destroy(h)

    @property
    def device_count(self) -> int:
        return lib().pire_hip_multi_device_count(self._h)

    @property
    def reduce_backend(self) -> str:
        return lib().pire_hip_multi_reduce_backend(self._h).decode()

    def run_shards(self, table: "Table", shards, flags=FLAG_BEGIN | FLAG_END, counts=True):
        """shards: one (text_ptr, n, len, stride, init_ptr, out_idx_ptr, out_final_ptr) per device (device pointers)."""
        arr = (Shard * len(shards))()
        for i, (text, n, length, stride, init, oi, of) in enumerate(shards):
            arr[i] = Shard(text or None, n, length, stride, init or None, oi or None, of or None)
        cnt = np.zeros(table.RegexpsCount + 2, dtype=np.uint64) if counts else None
        _check(lib().pire_hip_multi_run_strided(self._h, table._h, arr, flags, _np_ptr(cnt)))
        return cnt

    def run_offset_shards(self, table: "Table", shards, flags=FLAG_BEGIN | FLAG_END, counts=True):
        """shards: one (text_ptr, offsets_ptr, n, init_ptr, out_idx_ptr, out_final_ptr) per device (device pointers)."""
        arr = (ShardOffsets * len(shards))()
        for i, (text, offs, n, init, oi, of) in enumerate(shards):
            arr[i] = ShardOffsets(text or None, offs or None, n, init or None, oi or None, of or None)
        cnt = np.zeros(table.RegexpsCount + 2, dtype=np.uint64) if counts else None
        _check(lib().pire_hip_multi_run(self._h, table._h, arr, flags, _np_ptr(cnt)))
        return cnt

    def run_host(self, table: "Table", text, offsets, flags=FLAG_BEGIN | FLAG_END, init_idx=None):
        """A host batch of ragged strings sharded over the devices by BYTES; (idx, fin, counts) in string order."""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray))
                                    else text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        idx = np.empty(n, dtype=np.uint32)
        fin = np.empty(n, dtype=np.uint8)
        init = None if init_idx is None else np.ascontiguousarray(init_idx, dtype=np.uint32)
        cnt = np.zeros(table.RegexpsCount + 2, dtype=np.uint64)
        _check(lib().pire_hip_multi_run_host(self._h, table._h, text.ctypes.data if text.size else None,
                                             offsets.ctypes.data, n, flags, _np_ptr(init), idx.ctypes.data,
                                             fin.ctypes.data, cnt.ctypes.data))
        return idx, fin, cnt

    def last_split(self):
        """First string of every shard of the last host-pointer call, then n."""
        out = (C.c_uint64 * (self.device_count + 1))()
        k = lib().pire_hip_multi_last_split(self._h, out, self.device_count + 1)
        _check(min(k, 0))
        return [int(out[i]) for i in range(k)]

    def run_strided_host(self, table: "Table", text2d: np.ndarray, flags=FLAG_BEGIN | FLAG_END, init_idx=None):
        text2d = np.ascontiguousarray(text2d, dtype=np.uint8)
        n, length = text2d.shape
        idx = np.empty(n, dtype=np.uint32)
        fin = np.empty(n, dtype=np.uint8)
        init = None if init_idx is None else np.ascontiguousarray(init_idx, dtype=np.uint32)
        cnt = np.zeros(table.RegexpsCount + 2, dtype=np.uint64)
        _check(lib().pire_hip_multi_run_strided_host(self._h, table._h, text2d.ctypes.data if text2d.size else None, n,
                                                     length, length, flags, _np_ptr(init), idx.ctypes.data,
                                                     fin.ctypes.data, cnt.ctypes.data))
        return idx, fin, cnt


def run_pair_strided_device(t1: "Table", t2: "Table", text_ptr, n, length, stride, flags, out_idx1_ptr=0, out_idx2_ptr=0,
                            out_final_ptr=0, stream=0):
    """Pire::Run(sc1, sc2, ...) over device-resident fixed-length records: one fused pass (pair.hip)."""
    _check(lib().pire_hip_run_pair_strided(t1._h, t2._h, text_ptr or None, n, length, stride, flags | FLAG_ON_DEVICE,
                                           out_idx1_ptr or None, out_idx2_ptr or None, out_final_ptr or None, stream or None))


def run_pair_device(t1: "Table", t2: "Table", text_ptr, offsets_ptr, n, flags, out_idx1_ptr=0, out_idx2_ptr=0,
                    out_final_ptr=0, stream=0):
    _check(lib().pire_hip_run_pair(t1._h, t2._h, text_ptr or None, offsets_ptr or None, n, flags | FLAG_ON_DEVICE,
                                   out_idx1_ptr or None, out_idx2_ptr or None, out_final_ptr or None, stream or None))


def build_info() -> str:
    return lib().pire_hip_build_info().decode()


def last_kernel() -> str:
    return lib().pire_hip_last_kernel().decode()


def selftested_kernels():
    """The kernel names that have passed a first-use self-test in this process."""
    return [k for k in lib().pire_hip_selftested_kernels().decode().split(",") if k]


def last_kernel_symbol() -> str:
    return lib().pire_hip_last_kernel_symbol().decode()


def set_timing(enabled: bool):
    lib().pire_hip_set_timing(1 if enabled else 0)


def last_kernel_ms() -> float:
    return float(lib().pire_hip_last_kernel_ms())


CORPUS_MAX_PLANTS = 16
CORPUS_PLANT_BYTES = 64


class CorpusPlants(C.Structure):
    """pire_hip_corpus_plants (include/pire_hip.h)."""
    _fields_ = [
        ("nplants", C.c_uint32),
        ("len", C.c_uint32 * CORPUS_MAX_PLANTS),
        ("at_tail", C.c_uint32 * CORPUS_MAX_PLANTS),
        ("bytes", (C.c_uint8 * CORPUS_PLANT_BYTES) * CORPUS_MAX_PLANTS),
    ]


def make_plants(plants) -> CorpusPlants:
    """plants: sequence of (witness_bytes, at_tail_bool)."""
    p = CorpusPlants()
    if len(plants) > CORPUS_MAX_PLANTS:
        raise ValueError("too many plants")
    p.nplants = len(plants)
    for i, (w, tail) in enumerate(plants):
        if len(w) > CORPUS_PLANT_BYTES:
            raise ValueError("plant too long")
        p.len[i] = len(w)
        p.at_tail[i] = 1 if tail else 0
        for k, b in enumerate(w):
            p.bytes[i][k] = b
    return p


def corpus_fill_device(out_ptr: int, seed: int, first: int, count: int, length: int, stride: int, plants=None,
                       stream: int = 0):
    """Generate the synthetic corpus in device memory (plants: a CorpusPlants of this module or of oracle.binding --
    the same layout -- or None)."""
    p = C.byref(plants) if plants is not None else None
    _check(lib().pire_hip_corpus_fill(out_ptr, seed, first, count, length, stride, p, stream or None))
