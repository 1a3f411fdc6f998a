"""bgsa_amd — Python view of the MI355X backend for BGSA's all-pairs bit-parallel alignment.

The product is the C-ABI shared library `libbgsa_hip.so` (include/bgsa_hip.h, built from
bgsa_amd/csrc/*.hip for gfx950).  This module only loads it with ctypes and adds thin helpers
that hold device memory in torch tensors (plumbing: allocation, streams, torch.distributed).
There is no CPU fallback: if the library is missing, importing the compute API raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
# BGSA_HIP_LIB: another build of the same library (A/B measurements of generator variants)
LIB_PATH = Path(os.environ["BGSA_HIP_LIB"]) if os.environ.get("BGSA_HIP_LIB") else HERE / "libbgsa_hip.so"
# the A/B flavour of the same library (`make -C bgsa_amd/csrc ab`): additionally every measured-and-not-adopted kernel a
# measurement knob can select and three more BitPAl score sets; the knob tests and A/B scripts load it through BGSA_HIP_LIB
LIB_AB_PATH = HERE / "libbgsa_hip_ab.so"
INCLUDE = HERE.parent / "include" / "bgsa_hip.h"

ALGO_MYERS, ALGO_BANDED, ALGO_BITPAL = 0, 1, 2
DISTANCE_BEYOND = -2   # BGSA_HIP_DISTANCE_BEYOND: align_pairs_banded's distance of a pair beyond max_distance
V_NUM = 64

_lib = None


class Params(ctypes.Structure):
    """bgsa_hip_params_t of include/bgsa_hip.h: everything a scoring call reads, as one value."""
    _fields_ = [("algo", ctypes.c_int), ("alignment", ctypes.c_int), ("match", ctypes.c_int),
                ("mismatch", ctypes.c_int), ("gap", ctypes.c_int), ("k", ctypes.c_int)]


class SamBatch(ctypes.Structure):
    """bgsa_hip_sam_batch_t of include/bgsa_hip.h "SAM records": what the two record passes read, device pointers and extents."""
    _fields_ = [("d_reads", ctypes.c_void_p), ("d_quals", ctypes.c_void_p), ("read_stride", ctypes.c_int64), ("n_read_rows", ctypes.c_int64),
                ("d_names", ctypes.c_void_p), ("d_name_offsets", ctypes.c_void_p), ("n_names", ctypes.c_int64), ("names_bytes", ctypes.c_int64),
                ("d_rname", ctypes.c_void_p), ("rname_len", ctypes.c_int64), ("d_reference", ctypes.c_void_p), ("ref_len", ctypes.c_int64),
                ("d_runs", ctypes.c_void_p), ("n_run_rows", ctypes.c_int64), ("cigar_cap", ctypes.c_int64),
                ("d_read_row", ctypes.c_void_p), ("d_name_of", ctypes.c_void_p), ("d_runs_row", ctypes.c_void_p),
                ("d_read_len", ctypes.c_void_p), ("d_strand", ctypes.c_void_p), ("d_ref_begin", ctypes.c_void_p), ("d_ref_end", ctypes.c_void_p),
                ("d_distance", ctypes.c_void_p), ("d_n_ops", ctypes.c_void_p), ("d_flag", ctypes.c_void_p), ("d_mapq", ctypes.c_void_p),
                ("d_rnext", ctypes.c_void_p), ("d_pnext", ctypes.c_void_p), ("d_tlen", ctypes.c_void_p)]


class SamContigs(ctypes.Structure):
    """bgsa_hip_sam_contigs_t of include/bgsa_hip.h "a reference of several contigs": the name table and the layout, device pointers."""
    _fields_ = [("d_names", ctypes.c_void_p), ("d_name_offsets", ctypes.c_void_p), ("names_bytes", ctypes.c_int64),
                ("d_starts", ctypes.c_void_p), ("d_lens", ctypes.c_void_p), ("n_contigs", ctypes.c_int64)]


class BgsaHipError(RuntimeError):
    pass


def build_library(verbose: bool = False) -> Path:
    """Compile libbgsa_hip.so in-tree (hipcc --offload-arch=gfx950).  Works without a GPU."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.run(["make", "-C", str(HERE / "csrc"), "-j8", "all", "ab"], check=True, stdout=out)
    subprocess.run(["make", "-C", str(HERE / "host")], check=True, stdout=out)  # aligner, convert (C)
    return LIB_PATH


def declared_symbols() -> list[str]:
    """Function names declared in include/bgsa_hip.h (used by the symbol-export test)."""
    import re
    text = INCLUDE.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)  # preprocessor lines
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)
    return sorted(set(n for n in names if n not in ("defined",)))


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise BgsaHipError(
            f"{LIB_PATH} is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C bgsa_amd/csrc`.  There is no CPU fallback for the HIP path.")
    # torch first: it bundles its own ROCm runtime, and the process must end up with ONE HIP/HSA
    # runtime.  Loaded in the other order (this library pulling in /opt/rocm's libamdhip64 before torch
    # brings its libhsa-runtime64) the runtime finds no device.
    import torch  # noqa: F401
    L = ctypes.CDLL(str(LIB_PATH))
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    L.bgsa_hip_last_error.restype = ctypes.c_char_p
    L.bgsa_hip_select_algorithm.argtypes = [i32]
    L.bgsa_hip_select_scores.argtypes = [i32, i32, i32]
    L.bgsa_hip_select_alignment.argtypes = [i32]
    ip = ctypes.POINTER(i32)
    L.bgsa_hip_score_set.argtypes = [i32, ip, ip, ip, ip]
    L.bgsa_hip_word_num.argtypes = [i32, i32, i32, i32]
    L.bgsa_hip_group_words.argtypes = [i32, i32, i32]
    L.bgsa_hip_group_words.restype = sz
    L.bgsa_hip_handle_reads_dev.argtypes = [i32, vp, i64, i32, i64, i32, i32, vp, vp]
    L.bgsa_hip_map_queries_dev.argtypes = [vp, i64, vp]
    L.bgsa_hip_cal_align_score_dev.argtypes = [i32, vp, vp, vp, i32, i32, i64, i32, i32, i32, i32, vp, sz, vp]
    L.bgsa_hip_workspace_bytes.argtypes = [i32, i32, i32, i32]
    L.bgsa_hip_workspace_bytes.restype = sz
    pp = ctypes.POINTER(Params)
    L.bgsa_hip_current_params.argtypes = [pp]
    L.bgsa_hip_workspace_bytes_ex.argtypes = [pp, i32, i32, i32]
    L.bgsa_hip_workspace_bytes_ex.restype = sz
    L.bgsa_hip_cal_align_score_ex.argtypes = [pp, vp, vp, vp, i32, i32, i64, i32, i32, i32, vp, sz, vp]
    L.bgsa_hip_hits_workspace_bytes.argtypes = [i32, i64, i32, i32]
    L.bgsa_hip_hits_workspace_bytes.restype = sz
    L.bgsa_hip_top_hits_dev.argtypes = [vp, i32, i32, i64, i64, i64, i32, i32, i32, vp, vp, vp, sz, vp]
    L.bgsa_hip_threshold_hits_dev.argtypes = [vp, i32, i32, i64, i64, i64, i32, i32, i32, i64, vp, vp, vp, vp, sz, vp]
    L.bgsa_hip_align_pairs_workspace_bytes.argtypes = [i32, i32, i64]
    L.bgsa_hip_align_pairs_workspace_bytes.restype = sz
    L.bgsa_hip_align_pairs_min_workspace_bytes.argtypes = [i32, i32]
    L.bgsa_hip_align_pairs_min_workspace_bytes.restype = sz
    L.bgsa_hip_myers_align_pairs_dev.argtypes = [vp, vp, i32, i32, i64, i32, vp, vp, i64, i32, i64, vp, vp, vp, i32, vp, sz, vp]
    L.bgsa_hip_trace_pairs_dev.argtypes = [pp, vp, vp, i32, i32, i64, i32, vp, vp, i64, i32, i64, vp, vp, vp, vp, i32, vp, sz, vp]
    # mixed-length buckets (an older build loaded through BGSA_HIP_LIB for an A/B lacks them: calling one then raises AttributeError)
    for name, types in (("bgsa_hip_cal_align_score_lens_ex", [pp, vp, vp, vp, vp, i32, i32, i64, i32, i32, i32, vp, sz, vp]),
                        ("bgsa_hip_myers_align_pairs_lens_dev", [vp, vp, vp, i32, i32, i64, i32, vp, vp, i64, i32, i64, vp, vp, vp, i32, vp, sz, vp]),
                        ("bgsa_hip_trace_pairs_lens_dev", [pp, vp, vp, vp, i32, i32, i64, i32, vp, vp, i64, i32, i64, vp, vp, vp, vp, i32, vp, sz, vp])):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
    # read placement on mixed-length buckets, Myers semi-global with per-lane lengths (the same: an older build lacks them)
    for name, types in (("bgsa_hip_myers_place_score_lens_dev", [vp, vp, vp, vp, i32, i32, i64, i32, i32, i32, vp, sz, vp]),
                        ("bgsa_hip_myers_place_trace_pairs_lens_dev",
                         [vp, vp, vp, i32, i32, i64, i32, vp, vp, i64, i32, i64, vp, vp, vp, vp, i32, vp, sz, vp])):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
    # band-limited pair alignment (the same: an older build lacks it)
    for name, types, restype in (("bgsa_hip_align_pairs_band_words", [i32, i32, i32], i32),
                                 ("bgsa_hip_align_pairs_banded_min_workspace_bytes", [i32, i32, i32], sz),
                                 ("bgsa_hip_align_pairs_banded_workspace_bytes", [i32, i32, i32, i64], sz),
                                 ("bgsa_hip_myers_align_pairs_banded_dev",
                                  [vp, vp, i32, i32, i64, i32, vp, vp, i64, i32, i64, i32, vp, vp, vp, i32, vp, sz, vp], i32)):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = restype
    # band-limited semi-global placement (the same: an older build lacks it)
    for name, types, restype in (("bgsa_hip_place_pairs_band_words", [i32, i32], i32),
                                 ("bgsa_hip_place_pairs_banded_min_workspace_bytes", [i32, i32, i32], sz),
                                 ("bgsa_hip_place_pairs_banded_workspace_bytes", [i32, i32, i32, i64], sz),
                                 ("bgsa_hip_myers_place_pairs_banded_dev",
                                  [vp, vp, i32, i32, i64, i32, vp, vp, i64, i32, i64, i32, vp, vp, vp, vp, i32, vp, sz, vp], i32)):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = restype
    # hit lists per subject (the same: an older build lacks them)
    for name, types, restype in (("bgsa_hip_query_hits_workspace_bytes", [i32, i64, i32, i32], sz),
                                 ("bgsa_hip_top_queries_dev", [vp, i32, i32, i64, i64, i32, i32, i32, i32, vp, vp, vp, sz, vp], i32),
                                 ("bgsa_hip_threshold_queries_dev",
                                  [vp, i32, i32, i64, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp], i32)):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = restype
    # a reference as the query set (the same: an older build lacks them)
    for name, types, restype in (("bgsa_hip_reference_window_count", [i64, i32, i32], i64),
                                 ("bgsa_hip_reference_window_start", [i64, i32, i32, i64], i64),
                                 ("bgsa_hip_reference_windows_dev", [vp, i64, i32, i32, vp, i64, i64, vp, vp], i32),
                                 ("bgsa_hip_reference_placements_dev",
                                  [i64, i32, i32, vp, i64, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp], i32)):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = restype
    # seeded read mapping (the same: an older build lacks them)
    seed = [i64, i32, i32, vp, vp, i32, vp, i32, i64, i32, i32]   # the shape, the index, the reads, the bound, both_strands
    for name, types, restype in (("bgsa_hip_seed_index_offsets", [i32], i64),
                                 ("bgsa_hip_seed_index_workspace_bytes", [i64, i32], sz),
                                 ("bgsa_hip_seed_index_build_dev", [vp, i64, i32, vp, vp, vp, sz, vp], i32),
                                 ("bgsa_hip_seed_count_candidates_dev", seed + [i64, vp, vp], i32),
                                 ("bgsa_hip_seed_emit_candidates_dev", seed + [vp, vp, i64, vp, vp, vp], i32),
                                 ("bgsa_hip_reference_verify_workspace_bytes", [i32, i32, i64], sz),
                                 ("bgsa_hip_reference_verify_kernel_name", [i32, i32], ctypes.c_char_p),
                                 ("bgsa_hip_reference_verify_pairs_dev",
                                  [vp, i64, i32, i32, vp, i32, i64, i32, vp, vp, i64, i64, vp, vp, sz, vp], i32),
                                 ("bgsa_hip_seed_select_dev", [vp, vp, vp, i64, i32, i32, vp, vp, vp], i32),
                                 # every read at its own length: d_read_lens follows the reads / the planes
                                 ("bgsa_hip_seed_count_candidates_lens_dev", seed[:7] + [vp] + seed[7:] + [i64, vp, vp], i32),
                                 ("bgsa_hip_seed_emit_candidates_lens_dev", seed[:7] + [vp] + seed[7:] + [vp, vp, i64, vp, vp, vp], i32),
                                 ("bgsa_hip_reference_verify_pairs_lens_dev",
                                  [vp, i64, i32, i32, vp, vp, i32, i64, i32, vp, vp, i64, i64, vp, vp, sz, vp], i32)):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = restype
    # paired reads (the same: an older build lacks them)
    for name, types, restype in (("bgsa_hip_pair_rescue_slots", [i64, i32, i32, i64], i64),
                                 ("bgsa_hip_pair_rescue_windows_dev", [i64, i32, i32, vp, vp, vp, vp, i64, i32, i32, i64, vp, vp], i32),
                                 ("bgsa_hip_pair_select_dev", [vp] * 5 + [i32] + [vp] * 5 + [i32, i64, i64, i64] + [vp] * 8, i32)):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = restype
    # SAM records (the same: an older build lacks them)
    for name, types in (("bgsa_hip_sam_mapq_dev", [vp, vp, i64, i32, i32, vp, vp, vp, vp, vp]),
                        ("bgsa_hip_sam_measure_dev", [ctypes.POINTER(SamBatch), i64, vp, vp, vp]),
                        ("bgsa_hip_sam_emit_dev", [ctypes.POINTER(SamBatch), i64, vp, vp, i64, vp, vp])):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = i32
    # BAM records and BGZF framing (the same: an older build lacks them)
    for name, types, restype in (("bgsa_hip_bam_measure_dev", [ctypes.POINTER(SamBatch), i64, vp, vp, vp], i32),
                                 ("bgsa_hip_bam_emit_dev", [ctypes.POINTER(SamBatch), i64, vp, vp, i64, vp, vp], i32),
                                 ("bgsa_hip_bam_measure_contigs_dev", [ctypes.POINTER(SamBatch), ctypes.POINTER(SamContigs), i64, vp, vp, vp], i32),
                                 ("bgsa_hip_bam_emit_contigs_dev", [ctypes.POINTER(SamBatch), ctypes.POINTER(SamContigs), i64, vp, vp, i64, vp, vp],
                                  i32),
                                 ("bgsa_hip_bgzf_framed_bytes", [i64, i32], i64),
                                 ("bgsa_hip_bgzf_frame_dev", [vp, i64, i32, vp, i64, vp], i32),
                                 ("bgsa_hip_bgzf_deflate_workspace_bytes", [i64, i32], i64),
                                 ("bgsa_hip_bgzf_deflate_dev", [vp, i64, i32, vp, i64, vp, vp, i64, vp], i32),
                                 ("bgsa_hip_bgzf_pack_dev", [vp, i32, i64, vp, vp, i64, vp, vp], i32)):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = restype
    # coordinate order and the BAI index (the same: an older build lacks them)
    for name, types, restype in (("bgsa_hip_bam_coordinates_dev", [ctypes.POINTER(SamBatch), i64] + [vp] * 7, i32),
                                 ("bgsa_hip_bam_coordinates_contigs_dev", [ctypes.POINTER(SamBatch), ctypes.POINTER(SamContigs), i64] + [vp] * 7,
                                  i32),
                                 ("bgsa_hip_bam_index_windows", [vp, i64, vp], i64),
                                 ("bgsa_hip_bam_index_marks_dev", [vp] * 4 + [i64, vp, i64, i32, vp, i64, vp, i64] + [vp] * 6, i32),
                                 ("bgsa_hip_bam_index_chunks_dev", [vp] * 6 + [i64, i64] + [vp] * 6, i32),
                                 # duplicate marking
                                 ("bgsa_hip_dup_keys_dev", [ctypes.POINTER(SamBatch), i64, i32, i32] + [vp] * 6, i32),
                                 ("bgsa_hip_dup_mark_dev", [vp, vp, vp, i64, i32, vp, vp, vp], i32),
                                 # the merge of many calls' records
                                 ("bgsa_hip_bam_gather_dev", [vp, i64, vp, i64, vp, vp, i64, i64, i64, i64, i64, vp, vp, vp, vp], i32),
                                 # the pileup of the records and its candidate sites
                                 ("bgsa_hip_pileup_dev", [ctypes.POINTER(SamBatch), i64, i32, i32, i32, vp, vp, vp], i32),
                                 ("bgsa_hip_pileup_site_blocks", [i64], i64),
                                 ("bgsa_hip_pileup_sites_count_dev", [vp, vp, i64, i32, i32, i32, vp, i64, vp], i32),
                                 ("bgsa_hip_pileup_sites_emit_dev", [vp, vp, i64, i32, i32, i32, vp, i64, i64] + [vp] * 8, i32)):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = restype
    # a reference of several contigs (the same: an older build lacks them)
    for name, types in (("bgsa_hip_contig_layout", [vp, i64, i32, i64, vp, vp]),
                        ("bgsa_hip_contig_clip_dev", [vp, vp, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
                        ("bgsa_hip_sam_measure_contigs_dev", [ctypes.POINTER(SamBatch), ctypes.POINTER(SamContigs), i64, vp, vp, vp]),
                        ("bgsa_hip_sam_emit_contigs_dev", [ctypes.POINTER(SamBatch), ctypes.POINTER(SamContigs), i64, vp, vp, i64, vp, vp])):
        if hasattr(L, name):
            getattr(L, name).argtypes = types
            getattr(L, name).restype = i32
    L.bgsa_hip_stream_faults.argtypes = [i32]
    L.bgsa_hip_debug_inject_stream_fault.argtypes = [i32]
    L.bgsa_hip_set_auto_resident.argtypes = [i32]
    L.bgsa_hip_set_strict_resident.argtypes = [i32]
    L.bgsa_hip_stale_ranges.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    L.bgsa_hip_bucket_resident.argtypes = [vp, sz, i32]
    L.bgsa_hip_bucket_release.argtypes = [vp]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.bgsa_hip_seam_stats.argtypes = [u64p, u64p, u64p]
    L.bgsa_hip_row_cache_stats.argtypes = [u64p, u64p]
    L.bgsa_hip_event_create.argtypes = [ctypes.POINTER(vp)]
    L.bgsa_hip_event_destroy.argtypes = [vp]
    L.bgsa_hip_event_record.argtypes = [vp, vp]
    L.bgsa_hip_event_synchronize.argtypes = [vp]
    L.bgsa_hip_event_elapsed_ms.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float)]
    L.bgsa_hip_stream_wait_event.argtypes = [vp, vp]
    L.bgsa_hip_query_stream.argtypes = [i32, vp, i32, i32, vp, i32]
    L.bgsa_hip_myers_band_stream.argtypes = [vp, i32, i32, vp, i32]
    L.bgsa_hip_myers_band_half.argtypes = [i32, i32]
    L.bgsa_hip_myers_band_stats.argtypes = [vp, i32]
    if hasattr(L, "bgsa_hip_myers_band_groups"):   # (an older build loaded through BGSA_HIP_LIB lacks it)
        L.bgsa_hip_myers_band_groups.argtypes = [i32, i64, i32, i32, i32]
    if hasattr(L, "bgsa_hip_myers_band_rescue"):   # (the same)
        L.bgsa_hip_myers_band_rescue.argtypes = [i32, i32, i32, i64]
        L.bgsa_hip_myers_band_rescue_half.argtypes = [i32]
        L.bgsa_hip_myers_band_rescue_stats.argtypes = [vp, i32]
    if hasattr(L, "bgsa_hip_myers_prefix_depths"):   # (the same)
        L.bgsa_hip_myers_prefix_depths.argtypes = [i32, i64, i32, i32, i32, i32, ip, i32]
        L.bgsa_hip_myers_band_segments.argtypes = [vp, i32, i32, ip, i32, vp, i32, ip]
    if hasattr(L, "bgsa_hip_myers_band_early"):   # (the same)
        L.bgsa_hip_myers_band_early.argtypes = [i32, i32, i32, i64, ip]
        L.bgsa_hip_myers_band_early_cuts.argtypes = [i32, i32, ip, ip]
        L.bgsa_hip_myers_band_early_segments.argtypes = [vp, i32, i32, ip, ip, i32, ip, i32, vp, i32, ip]
    L.bgsa_hip_kernel_name.argtypes = [i32, i32]
    L.bgsa_hip_kernel_name.restype = ctypes.c_char_p
    L.bgsa_hip_malloc.argtypes = [ctypes.POINTER(vp), sz]
    L.bgsa_hip_free.argtypes = [vp]
    L.bgsa_hip_malloc_host.argtypes = [ctypes.POINTER(vp), sz]
    L.bgsa_hip_free_host.argtypes = [vp]
    L.bgsa_hip_memcpy_h2d.argtypes = [vp, vp, sz, vp]
    L.bgsa_hip_memcpy_d2h.argtypes = [vp, vp, sz, vp]
    L.bgsa_hip_memset.argtypes = [vp, i32, sz, vp]
    L.bgsa_hip_stream_synchronize.argtypes = [vp]
    L.bgsa_hip_stream_create.argtypes = [ctypes.POINTER(vp)]
    L.bgsa_hip_stream_destroy.argtypes = [vp]
    L.bgsa_hip_set_device.argtypes = [i32]
    # host-buffer BGSA surface
    L.hip_handle_reads.argtypes = [vp, vp, i32, i64, i64]
    L.hip_handle_reads.restype = None
    L.hip_cal_align_score.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.hip_cal_align_score.restype = None
    L.align_hip.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
    L.align_hip.restype = None
    L.init_mapping_table.restype = None
    L.malloc_mem.argtypes = [ctypes.c_uint64]
    L.malloc_mem.restype = vp
    L.free_mem.argtypes = [vp]
    L.free_mem.restype = None
    _lib = L
    return L


def check(rc: int, what: str = "bgsa_hip") -> None:
    if rc != 0:
        raise BgsaHipError(f"{what}: rc={rc}: {lib().bgsa_hip_last_error().decode()}")


class SeqT(ctypes.Structure):
    """seq_t of include/bgsa_hip.h (reference original/BGSA_CPU/global.h:9-16)."""
    _fields_ = [("len", ctypes.c_int), ("size", ctypes.c_int64), ("count", ctypes.c_int64),
                ("extra_size", ctypes.c_int), ("extra_count", ctypes.c_int),
                ("content", ctypes.c_void_p)]


def score_sets() -> list[tuple[int, int, int]]:
    """The (match, mismatch, gap) sets BitPAl kernels were compiled for (Makefile BITPAL_SETS)."""
    out = []
    for i in range(lib().bgsa_hip_score_set_count()):
        m, x, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().bgsa_hip_score_set(i, ctypes.byref(m), ctypes.byref(x), ctypes.byref(g), None), "score_set")
        out.append((m.value, x.value, g.value))
    return out


def word_num(algo: int, qlen: int, slen: int, k: int = 0) -> int:
    return int(lib().bgsa_hip_word_num(algo, qlen, slen, k))


def group_words(algo: int, wn: int, k: int = 0) -> int:
    return int(lib().bgsa_hip_group_words(algo, wn, k))


def default_smallest(algo: int, scores=None) -> bool:
    """Whether the smaller score is the better one for hit selection: distances (the banded filter, Myers +distance)."""
    return algo == ALGO_BANDED or (algo == ALGO_MYERS and scores is not None and tuple(scores) == (0, 1, 1))


def pad_rows(rows: np.ndarray, multiple: int = V_NUM) -> tuple[np.ndarray, int]:
    """Pad the subject set to a multiple of 64 with all-'N' reads, as get_read_from_file does for
    the final bucket (reference original/BGSA_CPU/file.c:98-112).  Returns (rows, extra_count)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, length = rows.shape
    extra = (-n) % multiple
    if extra:
        rows = np.concatenate([rows, np.full((extra, length), ord("N"), dtype=np.uint8)])
    return rows, extra


def pad_ragged(subjects) -> tuple[np.ndarray, np.ndarray]:
    """Subjects of mixed lengths (byte strings or 1-D uint8 arrays) as one bucket: (rows[ns, max_len] uint8, lens[ns] int32),
    every subject padded behind its own end with 'N'.  What the pad holds never enters a score (DeviceAligner.set_subjects_ragged).
    Raises on an empty list and on an empty subject."""
    seqs = [np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.asarray(x, dtype=np.uint8)
            for x in subjects]
    if not seqs:
        raise BgsaHipError("pad_ragged: no subjects")
    for i, x in enumerate(seqs):
        if x.ndim != 1:
            raise BgsaHipError(f"pad_ragged: subject {i} is not one-dimensional")
        if x.size == 0:
            raise BgsaHipError(f"pad_ragged: subject {i} is empty")
    lens = np.array([x.size for x in seqs], dtype=np.int32)
    rows = np.full((len(seqs), int(lens.max())), ord("N"), dtype=np.uint8)
    for i, x in enumerate(seqs):
        rows[i, : x.size] = x
    return rows, lens


def bin_by_words(lens) -> list[np.ndarray]:
    """The caller's subject indices grouped by ceil(len / 32) — the 32-bit words a subject occupies, which is what a bucket's
    kernel width and cost follow —, ascending groups, the caller's order kept within a group."""
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if lens.size and lens.min() < 1:
        raise BgsaHipError("bin_by_words: a length is not positive")
    words = (lens + 31) // 32
    return [np.flatnonzero(words == w) for w in np.unique(words)]


def rows_to_buffer(rows: np.ndarray) -> np.ndarray:
    """[n, len] ASCII -> the reference's row buffer (len bytes + '\\n' per row), flat uint8."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, length = rows.shape
    buf = np.full((n, length + 1), ord("\n"), dtype=np.uint8)
    buf[:, :length] = rows
    return buf.reshape(-1)


# ------------------------------------------------------------------------------------------------
# Device-resident driver (torch tensors hold the HBM buffers)
# ------------------------------------------------------------------------------------------------

class DeviceAligner:
    """One subject bucket resident in HBM, scored against query tiles.

    Mirrors what cal_on_<arch> does per read bucket (reference original/BGSA_CPU/cal_cpu.c:
    252-401): preprocess the bucket once, then loop over query buckets calling the grid.
    """

    def __init__(self, algo: int = ALGO_MYERS, device: str = "cuda:0", k: int = 0, scores=None,
                 semi_global: bool = False):
        """scores: (match, mismatch, gap) for ALGO_BITPAL; None = the reference's 2 / -3 / -5.
        For ALGO_MYERS (0, 1, 1) reports +distance (generator -m 1) instead of -distance.
        semi_global (generator -s): ALGO_BITPAL — query end to end, free subject overhangs;
        ALGO_MYERS — subject end to end inside the query (the generator's orientations differ)."""
        import torch
        self.torch = torch
        self.algo, self.k = algo, int(k)
        self.scores = tuple(int(x) for x in scores) if scores is not None else None
        self.semi_global = bool(semi_global)
        if self.scores is not None and algo != ALGO_BITPAL and not (algo == ALGO_MYERS and self.scores in ((0, 1, 1), (0, -1, -1))):
            raise BgsaHipError("scores apply to ALGO_BITPAL; ALGO_MYERS only knows (0, -1, -1) and (0, 1, 1) = +distance")
        if self.semi_global and algo == ALGO_BANDED:
            raise BgsaHipError("semi_global is not defined for the banded filter")
        self.device = torch.device(device)
        if not torch.cuda.is_available():
            raise BgsaHipError("no GPU visible: the HIP path has no CPU fallback")
        torch.cuda.set_device(self.device)
        check(lib().bgsa_hip_set_device(self.device.index or 0), "set_device")
        self.out_dtype = torch.int8 if algo == ALGO_BANDED else torch.int16
        self.d_lens = None    # per-column subject lengths of a mixed-length bucket (set_subjects_ragged, set_reads_ragged)
        self.reads_ragged = False   # the bucket is one of set_reads_ragged: Myers semi-global with every read's own length

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def set_queries(self, queries: np.ndarray) -> None:
        """queries: [nq, qlen] uint8 ASCII.  Uploads the row buffer and maps it to 0..4 in place."""
        torch = self.torch
        q = np.ascontiguousarray(queries, dtype=np.uint8)
        self.nq, self.qlen = q.shape
        buf = rows_to_buffer(q)
        # 8 spare bytes: the kernel's scalar dword fetch of the last characters stays in bounds
        self.d_content = torch.zeros(buf.size + 8, dtype=torch.uint8, device=self.device)
        self.d_content[: buf.size].copy_(torch.from_numpy(buf))
        check(lib().bgsa_hip_map_queries_dev(self.d_content.data_ptr(), buf.size, self._stream()), "map_queries")

    def set_query_rows_device(self, d_content, nq: int, qlen: int) -> None:
        """The counterpart of set_subject_rows_device for queries: d_content is a contiguous uint8 device tensor that already
        holds nq MAPPED rows (codes 0..4) of qlen + 1 bytes each ('\\n' last), followed by at least 8 spare bytes (the kernels'
        scalar dword fetch of the last characters stays in bounds).  Nothing is copied or launched: the tensor is the aligner's
        query buffer from here on (bgsa_hip_reference_windows_dev writes such rows; bgsa_amd.reference.ReferenceMapper)."""
        torch = self.torch
        nq, qlen = int(nq), int(qlen)
        if nq < 1 or qlen < 1:
            raise BgsaHipError("set_query_rows_device: rc=-1: nq and qlen must be positive")
        if not isinstance(d_content, torch.Tensor) or d_content.dtype != torch.uint8 or d_content.device != self.device or \
                d_content.dim() != 1 or not d_content.is_contiguous() or d_content.numel() < nq * (qlen + 1) + 8:
            raise BgsaHipError(f"set_query_rows_device: rc=-1: d_content must be a contiguous 1-D uint8 tensor on {self.device} of at "
                               f"least nq * (qlen + 1) + 8 = {nq * (qlen + 1) + 8} bytes")
        self.nq, self.qlen, self.d_content = nq, qlen, d_content

    def _set_bucket(self, rows: np.ndarray, lens=None, qlen: int | None = None, reads_ragged: bool = False):
        """The one upload of a subject bucket: rows [n, slen] uint8 ASCII, padded here to a multiple of 64 with 'N' reads (extra,
        ns_real), packed as a row buffer, uploaded and preprocessed (set_subject_rows_device).  lens: None, or the n rows' own
        lengths (a mixed-length bucket; the pad columns get slen); reads_ragged marks such a bucket as one of set_reads_ragged.
        Returns (the device row buffer — ASCII, ns rows of slen + 1 bytes —, the device lengths or None): the aligner keeps the
        lengths and drops the rows, a caller that reads them again (ReferenceMapper's seed filter) keeps them."""
        torch = self.torch
        s, self.extra = pad_rows(rows)
        self.ns_real = rows.shape[0]
        d_rows = torch.from_numpy(rows_to_buffer(s)).to(self.device)
        d_lens = None
        if lens is not None:
            lens = np.concatenate([np.asarray(lens, dtype=np.int32), np.full(self.extra, s.shape[1], dtype=np.int32)])
            d_lens = torch.from_numpy(lens).to(self.device)
        self.set_subject_rows_device(d_rows, s.shape[0], s.shape[1], qlen, d_lens=d_lens)
        if reads_ragged:
            self.mark_reads_ragged()
        return d_rows, d_lens

    def set_subjects(self, subjects: np.ndarray, qlen: int | None = None) -> None:
        """subjects: [ns, slen] uint8 ASCII (padded here to a multiple of 64 with 'N' reads)."""
        self._set_bucket(subjects, qlen=qlen)

    def set_subjects_ragged(self, subjects, qlen: int | None = None) -> None:
        """subjects: byte strings or 1-D uint8 arrays of MIXED lengths, as one bucket of the longest one's width (pad_ragged, then
        padded to a multiple of 64 with 'N' reads of that width).  From here on score, top_hits, threshold_hits, align_pairs,
        align_hits, trace_pairs and trace_hits treat column c as the subject's own first lens[c] characters: scores, hit lists and
        edit scripts are those of the unpadded subject, bit for bit.  Global modes only (Myers -distance / +distance, BitPAl with
        any compiled set, subjects up to 1,024 bp): the banded filter and the semi-global modes raise rc=-2 at the first scoring
        call.  The certified Myers band is off for such a bucket (full rows).  If all lengths are equal this IS set_subjects: no
        lengths are passed and the band stays available.  Queries keep one length per aligner: group queries by length.  To keep a
        short read from being scored at the width of the longest, bin the subjects first (bin_by_words, align_all_pairs_ragged)."""
        rows, lens = pad_ragged(subjects)
        if (lens == lens[0]).all():
            return self.set_subjects(rows, qlen)
        self._set_bucket(rows, lens, qlen)

    def _reads_ragged_refusals(self, what: str) -> None:
        if self.algo != ALGO_MYERS or not self.semi_global or self.scores == (0, 1, 1):
            raise BgsaHipError(f"{what}: rc=-2: reads of mixed lengths are placed by the Myers unit-cost semi-global aligner only "
                               "(ALGO_MYERS, semi_global=True, not +distance; global modes: set_subjects_ragged)")

    def set_reads_ragged(self, reads, qlen: int | None = None) -> None:
        """reads: byte strings or 1-D uint8 arrays of MIXED lengths, up to 1,024 bp, as one bucket of the Myers semi-global aligner
        (the read end to end inside the query): packed as set_subjects_ragged packs (pad_ragged, then pad_rows; pad columns get the
        longest length).  From here on score() — and with it top_hits, threshold_hits, top_queries, threshold_queries — and
        trace_pairs / trace_hits treat column c as the read's own first lens[c] characters, bit for bit what a bucket of that one
        length reports (bgsa_hip_myers_place_score_lens_dev, bgsa_hip_myers_place_trace_pairs_lens_dev).  Only ALGO_MYERS with
        semi_global=True and not +distance: anything else raises rc=-2 before anything is allocated.  If all lengths are equal this
        IS set_subjects.  place_pairs_banded keeps refusing a mixed-length bucket.  To keep a short read from being scored at the
        width of the longest, bin the reads first (bin_by_words; ReferenceMapper.map_reads_ragged does)."""
        self._reads_ragged_refusals("set_reads_ragged")
        rows, lens = pad_ragged(reads)
        if (lens == lens[0]).all():
            return self.set_subjects(rows, qlen)
        if rows.shape[1] > 1024:
            raise BgsaHipError("set_reads_ragged: rc=-2: reads beyond 1,024 bp (word_num > 32) run as column blocks, which have no "
                               "per-lane form")
        self._set_bucket(rows, lens, qlen, reads_ragged=True)

    def mark_reads_ragged(self) -> None:
        """Marks the bucket set_subject_rows_device(..., d_lens=) has just set as one of set_reads_ragged: its lengths are reads' own
        lengths under the Myers semi-global aligner.  Every later set_subject* call clears the mark."""
        self._reads_ragged_refusals("mark_reads_ragged")
        if self.d_lens is None:
            raise BgsaHipError("mark_reads_ragged: rc=-1: the bucket has no lengths (set_subject_rows_device(..., d_lens=))")
        self.reads_ragged = True

    def set_subject_rows_device(self, d_rows, ns: int, slen: int, qlen: int | None = None, d_lens=None) -> None:
        """d_rows: uint8 device tensor holding ns rows of slen+1 bytes; ns % 64 == 0.  d_lens: None (every subject is slen long), or
        an int32 device tensor of ns subject lengths (a mixed-length bucket, slen the longest: set_subjects_ragged)."""
        torch = self.torch
        if d_lens is not None and (d_lens.dtype != torch.int32 or d_lens.numel() != int(ns) or not d_lens.is_contiguous()):
            raise BgsaHipError("set_subject_rows_device: d_lens must be a contiguous int32 tensor of ns entries")
        self.d_lens = d_lens
        self.reads_ragged = False
        self.ns, self.slen = int(ns), int(slen)
        qlen = self.qlen if qlen is None else qlen
        self.wn = word_num(self.algo, qlen, self.slen, self.k)
        n_words = group_words(self.algo, self.wn, self.k) * (self.ns // V_NUM)
        self.d_peq = torch.empty(n_words, dtype=torch.int32, device=self.device)
        check(lib().bgsa_hip_handle_reads_dev(self.algo, d_rows.data_ptr(), d_rows.numel(), self.slen,
                                              self.ns, self.wn, self.k, self.d_peq.data_ptr(),
                                              self._stream()), "handle_reads_dev")

    def params(self) -> Params:
        """This aligner's own scoring parameters (the *_ex entry points take them explicitly, so two
        aligners with different scores or modes never meet in the C ABI's process-global ints)."""
        if self.algo == ALGO_BITPAL:
            m, x, g = self.scores or (2, -3, -5)
        elif self.algo == ALGO_MYERS and self.scores == (0, 1, 1):
            m, x, g = 0, 1, 1            # generator -m 1: +distance
        else:
            m, x, g = 0, -1, -1
        return Params(self.algo, 1 if self.semi_global else 0, m, x, g, self.k)

    def score(self, ref_start: int = 0, ref_end: int | None = None, out=None):
        """Scores queries [ref_start, ref_end) against the resident bucket -> [nq_tile, ns] tensor."""
        torch = self.torch
        ref_end = self.nq if ref_end is None else ref_end
        if out is None:
            out = torch.empty((ref_end - ref_start, self.ns), dtype=self.out_dtype, device=self.device)
        p = self.params()
        need = int(lib().bgsa_hip_workspace_bytes_ex(ctypes.byref(p), self.qlen, self.slen, ref_end - ref_start))
        if getattr(self, "d_work", None) is None or self.d_work.numel() < need:
            self.d_work = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
        if self.d_lens is not None and self.reads_ragged:
            check(lib().bgsa_hip_myers_place_score_lens_dev(self.d_content.data_ptr(), self.d_peq.data_ptr(), out.data_ptr(),
                                                            self.d_lens.data_ptr(), self.qlen, self.slen, self.ns, ref_start, ref_end,
                                                            self.wn, self.d_work.data_ptr(), self.d_work.numel(), self._stream()),
                  "myers_place_score_lens_dev")
            return out
        if self.d_lens is not None:
            check(lib().bgsa_hip_cal_align_score_lens_ex(ctypes.byref(p), self.d_content.data_ptr(), self.d_peq.data_ptr(),
                                                         out.data_ptr(), self.d_lens.data_ptr(), self.qlen, self.slen, self.ns,
                                                         ref_start, ref_end, self.wn, self.d_work.data_ptr(),
                                                         self.d_work.numel(), self._stream()), "cal_align_score_lens_ex")
            return out
        check(lib().bgsa_hip_cal_align_score_ex(ctypes.byref(p), self.d_content.data_ptr(), self.d_peq.data_ptr(),
                                                out.data_ptr(), self.qlen, self.slen, self.ns, ref_start,
                                                ref_end, self.wn, self.d_work.data_ptr(),
                                                self.d_work.numel(), self._stream()), "cal_align_score_ex")
        return out

    # ---- hit selection: the score matrix never exists, only one reused tile of block_rows x ns ----------------------
    def _hit_blocks(self, block_rows: int):
        """Scores the resident bucket block_rows queries at a time into one reused tile; yields (lo, hi, tile rows)."""
        torch = self.torch
        block_rows = max(1, min(int(block_rows), self.nq))
        tile = getattr(self, "d_hit_tile", None)
        if tile is None or tile.shape != (block_rows, self.ns) or tile.dtype != self.out_dtype:
            self.d_hit_tile = tile = torch.empty((block_rows, self.ns), dtype=self.out_dtype, device=self.device)
        need = int(lib().bgsa_hip_hits_workspace_bytes(block_rows, self.ns, tile.element_size(), V_NUM))
        if getattr(self, "d_hit_work", None) is None or self.d_hit_work.numel() < need:
            self.d_hit_work = torch.empty(need, dtype=torch.uint8, device=self.device)
        for lo in range(0, self.nq, block_rows):
            hi = min(lo + block_rows, self.nq)
            yield lo, hi, self.score(lo, hi, out=tile[: hi - lo])

    def _hit_lists(self, into, shapes, what: str):
        """The output tensors of a selection call: fresh ones, or the caller's `into` (checked) to accumulate into."""
        torch = self.torch
        if into is None:
            return [torch.empty(shape, dtype=dtype, device=self.device) for shape, dtype in shapes], 0
        into = list(into)
        if len(into) != len(shapes):
            raise BgsaHipError(f"{what}: into= takes {len(shapes)} tensors")
        for t, (shape, dtype) in zip(into, shapes):
            if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                raise BgsaHipError(f"{what}: into= needs contiguous {dtype} tensors of shape {tuple(shape)} on {self.device}")
        return into, 1

    def top_hits(self, k_best: int, block_rows: int = 1000, smallest=None, subject_base: int = 0, into=None):
        """The k_best (1..64) best subjects of the resident bucket per query, best first, ties to the smaller subject id:
        (scores[nq, K] int32, subjects[nq, K] int64) device tensors; subjects are subject_base + index in the bucket, unused
        slots hold -1.  The bucket is scored block_rows queries at a time into one reused tile and each block is selected
        on the device (bgsa_hip_top_hits_dev).  into=(scores, subjects) of an earlier call: its entries join the
        candidates, so walking several buckets ends with the K best overall.  smallest=None follows the aligner."""
        torch = self.torch
        smallest = default_smallest(self.algo, self.scores) if smallest is None else bool(smallest)
        k_best = int(k_best)
        if not 1 <= k_best <= V_NUM:    # before any tensor is sized by it; the C call's own answer (BGSA_HIP_EUNSUPPORTED)
            raise BgsaHipError(f"top_hits: rc=-2: k_best must lie in 1..{V_NUM} (one wavefront holds the sorted list, one entry per lane)")
        (scores, subjects), accumulate = self._hit_lists(into, [((self.nq, k_best), torch.int32), ((self.nq, k_best), torch.int64)], "top_hits")
        for lo, hi, tile in self._hit_blocks(block_rows):
            check(lib().bgsa_hip_top_hits_dev(tile.data_ptr(), tile.element_size(), hi - lo, self.ns, self.ns_real, int(subject_base),
                                              k_best, int(smallest), accumulate, scores[lo:hi].data_ptr(), subjects[lo:hi].data_ptr(),
                                              self.d_hit_work.data_ptr(), self.d_hit_work.numel(), self._stream()), "top_hits_dev")
        return scores, subjects

    def threshold_hits(self, cutoff: int, cap_per_query: int, block_rows: int = 1000, smallest=None, subject_base: int = 0, into=None):
        """Every subject of the resident bucket at least as good as `cutoff`, per query in ascending subject order:
        (counts[nq] int32, scores[nq, cap] int32, subjects[nq, cap] int64) device tensors.  counts are the true numbers
        of hits even beyond cap_per_query; a row that overflows keeps its cap_per_query lowest-indexed hits.
        into=(counts, scores, subjects) of an earlier call: this bucket's hits are appended behind them."""
        torch = self.torch
        smallest = default_smallest(self.algo, self.scores) if smallest is None else bool(smallest)
        cap = int(cap_per_query)
        if cap < 1:
            raise BgsaHipError("threshold_hits: rc=-1: cap_per_query is not positive")
        (counts, scores, subjects), accumulate = self._hit_lists(
            into, [((self.nq,), torch.int32), ((self.nq, cap), torch.int32), ((self.nq, cap), torch.int64)], "threshold_hits")
        for lo, hi, tile in self._hit_blocks(block_rows):
            check(lib().bgsa_hip_threshold_hits_dev(tile.data_ptr(), tile.element_size(), hi - lo, self.ns, self.ns_real, int(subject_base),
                                                    int(cutoff), int(smallest), accumulate, cap, counts[lo:hi].data_ptr(),
                                                    scores[lo:hi].data_ptr(), subjects[lo:hi].data_ptr(),
                                                    self.d_hit_work.data_ptr(), self.d_hit_work.numel(), self._stream()), "threshold_hits_dev")
        return counts, scores, subjects

    # ---- hit lists per subject: the same tile reduced along its columns (bgsa_hip_top_queries_dev) -------------------------
    def _query_hit_work(self, block_rows: int, k_best: int):
        need = int(lib().bgsa_hip_query_hits_workspace_bytes(max(1, min(int(block_rows), self.nq)), self.ns, 1 if self.algo == ALGO_BANDED else 2, k_best))
        if getattr(self, "d_query_hit_work", None) is None or self.d_query_hit_work.numel() < need:
            self.d_query_hit_work = self.torch.empty(max(need, 8), dtype=self.torch.uint8, device=self.device)
        return self.d_query_hit_work

    def top_queries(self, k_best: int, block_rows: int = 1000, smallest=None, query_base: int = 0, into=None):
        """The k_best (1..64) best QUERIES per subject of the resident bucket, best first, ties to the smaller query id:
        (scores[ns_real, K] int32, queries[ns_real, K] int32) device tensors; queries are query_base + index in this aligner's
        query set, unused slots (fewer than K queries) hold -1 and the worst int32 of the direction.  The bucket is scored
        block_rows queries at a time into one reused tile and every block joins the lists on the device
        (bgsa_hip_top_queries_dev, accumulate from the second block on).  into=(scores, queries) of an earlier call: its
        entries join the candidates with their ids as stored, so several query sets (set_queries, another query_base) end with
        the K best overall.  Several subject buckets need no into=: their lists are concatenated.  smallest=None follows the
        aligner."""
        torch = self.torch
        smallest = default_smallest(self.algo, self.scores) if smallest is None else bool(smallest)
        k_best = int(k_best)
        if not 1 <= k_best <= V_NUM:    # before any tensor is sized by it; the C call's own answer (BGSA_HIP_EUNSUPPORTED)
            raise BgsaHipError(f"top_queries: rc=-2: k_best must lie in 1..{V_NUM}")
        shape = (self.ns_real, k_best)
        (scores, queries), accumulate = self._hit_lists(into, [(shape, torch.int32), (shape, torch.int32)], "top_queries")
        work = self._query_hit_work(block_rows, k_best)
        for lo, hi, tile in self._hit_blocks(block_rows):
            check(lib().bgsa_hip_top_queries_dev(tile.data_ptr(), tile.element_size(), hi - lo, self.ns, self.ns_real, int(query_base) + lo,
                                                 k_best, int(smallest), accumulate, scores.data_ptr(), queries.data_ptr(),
                                                 work.data_ptr(), work.numel(), self._stream()), "top_queries_dev")
            accumulate = 1
        return scores, queries

    def threshold_queries(self, cutoff: int, cap_per_subject: int, block_rows: int = 1000, smallest=None, query_base: int = 0, into=None):
        """Every query at least as good as `cutoff`, per subject of the resident bucket in ascending query order:
        (counts[ns_real] int32, scores[ns_real, cap] int32, queries[ns_real, cap] int32) device tensors.  counts are the true
        numbers of hits even beyond cap_per_subject; a subject that overflows keeps its cap_per_subject lowest-indexed hits,
        slots behind a subject's hits are left as they were.  into=(counts, scores, queries) of an earlier call: this query
        set's hits are appended behind them."""
        torch = self.torch
        smallest = default_smallest(self.algo, self.scores) if smallest is None else bool(smallest)
        cap = int(cap_per_subject)
        if not 1 <= cap < 2 ** 31:
            raise BgsaHipError("threshold_queries: rc=-1: cap_per_subject is not a positive int32")
        (counts, scores, queries), accumulate = self._hit_lists(
            into, [((self.ns_real,), torch.int32), ((self.ns_real, cap), torch.int32), ((self.ns_real, cap), torch.int32)], "threshold_queries")
        work = self._query_hit_work(block_rows, 1)
        for lo, hi, tile in self._hit_blocks(block_rows):
            check(lib().bgsa_hip_threshold_queries_dev(tile.data_ptr(), tile.element_size(), hi - lo, self.ns, self.ns_real,
                                                       int(query_base) + lo, int(cutoff), int(smallest), accumulate, cap, counts.data_ptr(),
                                                       scores.data_ptr(), queries.data_ptr(), work.data_ptr(), work.numel(),
                                                       self._stream()), "threshold_queries_dev")
            accumulate = 1
        return counts, scores, queries

    def query_hits_as_pairs(self, hit_queries, subject_base: int = 0):
        """The queries[ns_real, K] tensor of top_queries / threshold_queries as a pair list, built on the device:
        (pair_queries int32[ns_real * K], pair_subjects int64[ns_real * K]); entry [c, r] becomes the pair (hit_queries[c, r],
        subject_base + c).  An unused slot (query -1) becomes query 0 with subject -1, which align_pairs, align_pairs_banded and
        trace_pairs skip (a negative query on an owned pair would raise BGSA_HIP_FAULT_PAIR).  Both vectors go to those calls
        unchanged; their outputs reshape to [ns_real, K, ...].  Slots of threshold_queries behind a subject's count hold
        whatever the caller put there: fill the tensor with -1 first (into=)."""
        torch = self.torch
        hq = torch.as_tensor(hit_queries).to(device=self.device)
        if hq.dim() != 2 or hq.shape[0] != self.ns_real or hq.dtype not in (torch.int32, torch.int64):
            raise BgsaHipError(f"query_hits_as_pairs: hit_queries must be an integer tensor [ns_real = {self.ns_real}, K]")
        used = hq >= 0
        columns = torch.arange(self.ns_real, dtype=torch.int64, device=self.device).add_(int(subject_base)).unsqueeze(1).expand_as(hq)
        pair_queries = torch.where(used, hq, torch.zeros_like(hq)).to(torch.int32).contiguous().view(-1)
        pair_subjects = torch.where(used, columns, torch.full_like(columns, -1)).contiguous().view(-1)
        return pair_queries, pair_subjects

    # ---- edit scripts of selected pairs (bgsa_hip_myers_align_pairs_dev) ----------------------------------------------
    def align_pairs(self, pair_queries, pair_subjects, cigar_cap=None, subject_base: int = 0, into=None, workspace_bytes=None):
        """The canonical edit script of every pair (pair_queries[p], pair_subjects[p]) against the resident bucket:
        (distance[n] int32, n_ops[n] int32, cigar[n, cap] uint32 runs `length << 4 | BAM op` held as int32) device tensors.
        Subject ids are as the hit lists report them (column = id - subject_base); a pair whose subject is -1 or belongs to
        another bucket is left as it was — fresh outputs hold distance -1, n_ops 0 and cigar 0 there.  into= the triple of
        an earlier call, for walking buckets.  cigar_cap=None: qlen + slen, which can never overflow; n_ops is the true
        number of runs even beyond the cap.  workspace_bytes: None = what all pairs need in one pass (at most 1 GiB), a
        size from bgsa_hip_align_pairs_min_workspace_bytes() up = that much (more chunks), 0 = the library's own scratch.
        Myers global only: any other aligner raises, and so does (0, 1, 1) +distance — the alignment is the same."""
        self._myers_global_only("align_pairs")
        pq, ps, n, cap, (distance, n_ops, cigar) = self._pair_lists("align_pairs", pair_queries, pair_subjects, cigar_cap, into)
        if n == 0:
            return distance, n_ops, cigar
        if workspace_bytes is None:
            workspace_bytes = int(lib().bgsa_hip_align_pairs_workspace_bytes(self.qlen, self.slen, n))
        work, work_bytes = self._align_workspace(workspace_bytes)
        if self.d_lens is not None:
            check(lib().bgsa_hip_myers_align_pairs_lens_dev(self.d_content.data_ptr(), self.d_peq.data_ptr(), self.d_lens.data_ptr(),
                                                            self.qlen, self.slen, self.ns, self.wn, pq.data_ptr(), ps.data_ptr(), n,
                                                            self.nq, int(subject_base), distance.data_ptr(), n_ops.data_ptr(),
                                                            cigar.data_ptr(), cap, work, work_bytes, self._stream()),
                  "myers_align_pairs_lens_dev")
            return distance, n_ops, cigar
        check(lib().bgsa_hip_myers_align_pairs_dev(self.d_content.data_ptr(), self.d_peq.data_ptr(), self.qlen, self.slen, self.ns, self.wn,
                                                   pq.data_ptr(), ps.data_ptr(), n, self.nq, int(subject_base), distance.data_ptr(),
                                                   n_ops.data_ptr(), cigar.data_ptr(), cap, work, work_bytes, self._stream()),
              "myers_align_pairs_dev")
        return distance, n_ops, cigar

    def align_hits(self, hit_subjects, cigar_cap=None, subject_base: int = 0, into=None, workspace_bytes=None):
        """align_pairs for the subjects[nq, K] tensor of top_hits / threshold_hits: row q holds subjects of query q (the
        query index is built on the device).  Returns (distance[nq, K], n_ops[nq, K], cigar[nq, K, cap]); unused slots
        (subject -1) keep distance -1, n_ops 0.  into= the triple of an earlier call, for walking buckets."""
        pq, ps, cigar_cap, into, (nq, k) = self._hits_as_pairs("align_hits", hit_subjects, cigar_cap, into)
        distance, n_ops, cigar = self.align_pairs(pq, ps, cigar_cap, subject_base, into, workspace_bytes)
        return distance.view(nq, k), n_ops.view(nq, k), cigar.view(nq, k, -1)

    # what align_pairs / align_hits and their band-limited counterparts share: the refusal, the lists, the workspace
    def _myers_global_only(self, what: str) -> None:
        if self.algo != ALGO_MYERS or self.semi_global or self.scores == (0, 1, 1):
            raise BgsaHipError(f"{what}: rc=-2: only Myers unit-cost global alignment is traced back (no semi-global mode, no "
                               "BitPAl score sets, no banded filter; +distance aligns the same as -distance: use that aligner)")

    def _pair_lists(self, what: str, pair_queries, pair_subjects, cigar_cap, into):
        """(pair queries int32[n], pair subjects int64[n], n, cap, (distance, n_ops, cigar)): the outputs fresh (-1 / 0 / 0) or the
        caller's `into`, checked."""
        torch = self.torch
        pq = torch.as_tensor(pair_queries).to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        ps = torch.as_tensor(pair_subjects).to(device=self.device, dtype=torch.int64).contiguous().reshape(-1)
        if pq.numel() != ps.numel():
            raise BgsaHipError(f"{what}: pair_queries and pair_subjects differ in length")
        n = pq.numel()
        cap = self.qlen + self.slen if cigar_cap is None else int(cigar_cap)
        if cap < 1:
            raise BgsaHipError(f"{what}: rc=-1: cigar_cap is not positive")
        shapes = [((n,), torch.int32), ((n,), torch.int32), ((n, cap), torch.int32)]
        if into is None:
            outs = tuple(torch.full(shape, fill, dtype=dtype, device=self.device) for (shape, dtype), fill in zip(shapes, (-1, 0, 0)))
        else:
            outs, _ = self._hit_lists(into, shapes, what)
        return pq, ps, n, cap, tuple(outs)

    def _align_workspace(self, workspace_bytes: int):
        """(device pointer, bytes) of the aligner's own pair workspace grown to workspace_bytes; (None, 0) = the library's scratch."""
        if not workspace_bytes:
            return None, 0
        if getattr(self, "d_align_work", None) is None or self.d_align_work.numel() < workspace_bytes:
            self.d_align_work = self.torch.empty(int(workspace_bytes), dtype=self.torch.uint8, device=self.device)
        return self.d_align_work.data_ptr(), int(workspace_bytes)

    def _hits_as_pairs(self, what: str, hit_subjects, cigar_cap, into):
        """A subjects[nq, K] tensor as a pair list: (pair queries, pair subjects, cigar_cap, into flattened, (nq, K))."""
        torch = self.torch
        hs = torch.as_tensor(hit_subjects).to(device=self.device, dtype=torch.int64)
        if hs.dim() != 2 or hs.shape[0] != self.nq:
            raise BgsaHipError(f"{what}: hit_subjects must be [nq = {self.nq}, K]")
        nq, k = hs.shape
        pq = torch.arange(nq, dtype=torch.int32, device=self.device).repeat_interleave(k)
        if into is not None:
            into = list(into)
            if len(into) != 3 or any(not t.is_contiguous() for t in into) or tuple(into[0].shape) != (nq, k) or \
                    tuple(into[1].shape) != (nq, k) or into[2].dim() != 3 or tuple(into[2].shape[:2]) != (nq, k):
                raise BgsaHipError(f"{what}: into= needs contiguous tensors of shape ({nq}, {k}), ({nq}, {k}), ({nq}, {k}, cap)")
            if cigar_cap is None:
                cigar_cap = into[2].shape[2]
            into = (into[0].view(-1), into[1].view(-1), into[2].view(nq * k, -1))
        return pq, hs.contiguous().view(-1), cigar_cap, into, (nq, k)

    # ---- the same within a distance bound, subjects of any length (bgsa_hip_myers_align_pairs_banded_dev) ------------------
    def align_pairs_banded(self, pair_queries, pair_subjects, max_distance: int, cigar_cap=None, subject_base: int = 0, into=None,
                           workspace_bytes=None):
        """align_pairs with the history limited to the band of max_distance: subjects of any length the scoring kernels
        take.  Same tensors and ownership rules; a pair whose distance is <= max_distance gets exactly align_pairs'
        distance, n_ops and runs, any other owned pair distance DISTANCE_BEYOND (-2), n_ops 0 and an untouched cigar row.
        max_distance is what the caller already knows: the cutoff of threshold_hits, the worst distance of top_hits.
        workspace_bytes: None = what all pairs need in one pass (at most 1 GiB), a size from
        bgsa_hip_align_pairs_banded_min_workspace_bytes() up = that much (more chunks), 0 = the library's own scratch.
        Myers global only, one subject length per bucket (no set_subjects_ragged)."""
        self._myers_global_only("align_pairs_banded")
        if self.d_lens is not None:
            raise BgsaHipError("align_pairs_banded: rc=-2: a bucket of mixed read lengths has no band-limited variant (one (m, n) "
                               "per window schedule): use align_pairs up to 1,024 bp")
        max_distance = min(int(max_distance), 2 ** 31 - 1)
        if max_distance < 0:
            raise BgsaHipError("align_pairs_banded: rc=-1: max_distance is negative")
        pq, ps, n, cap, (distance, n_ops, cigar) = self._pair_lists("align_pairs_banded", pair_queries, pair_subjects, cigar_cap, into)
        if n == 0:
            return distance, n_ops, cigar

        def call(n_pairs, work, work_bytes):
            check(lib().bgsa_hip_myers_align_pairs_banded_dev(self.d_content.data_ptr(), self.d_peq.data_ptr(), self.qlen, self.slen, self.ns,
                                                              self.wn, pq.data_ptr(), ps.data_ptr(), n_pairs, self.nq, int(subject_base),
                                                              max_distance, distance.data_ptr(), n_ops.data_ptr(), cigar.data_ptr(), cap,
                                                              work, work_bytes, self._stream()),
                  "myers_align_pairs_banded_dev")
        if workspace_bytes is None:
            call(0, None, 0)   # an empty list runs the C call's checks alone: a window too wide is refused before a workspace is allocated for it
            workspace_bytes = int(lib().bgsa_hip_align_pairs_banded_workspace_bytes(self.qlen, self.slen, max_distance, n))
        call(n, *self._align_workspace(workspace_bytes))
        return distance, n_ops, cigar

    def align_hits_banded(self, hit_subjects, max_distance: int, cigar_cap=None, subject_base: int = 0, into=None, workspace_bytes=None):
        """align_pairs_banded for the subjects[nq, K] tensor of top_hits / threshold_hits, as align_hits is for align_pairs:
        (distance[nq, K], n_ops[nq, K], cigar[nq, K, cap]); unused slots (subject -1) keep distance -1, n_ops 0."""
        pq, ps, cigar_cap, into, (nq, k) = self._hits_as_pairs("align_hits_banded", hit_subjects, cigar_cap, into)
        distance, n_ops, cigar = self.align_pairs_banded(pq, ps, max_distance, cigar_cap, subject_base, into, workspace_bytes)
        return distance.view(nq, k), n_ops.view(nq, k), cigar.view(nq, k, -1)

    # ---- score, span and edit script of selected pairs, every aligner with an alignment (bgsa_hip_trace_pairs_dev) --------
    def _trace_refusals(self, what: str) -> None:
        # the C call's own answers (BGSA_HIP_EUNSUPPORTED), given before anything is allocated or launched
        if self.algo == ALGO_BANDED:
            raise BgsaHipError(f"{what}: rc=-2: the banded filter's pairs are not traced back")
        if self.algo == ALGO_MYERS and self.scores == (0, 1, 1):
            raise BgsaHipError(f"{what}: rc=-2: Myers +distance (0, 1, 1) aligns the same as -distance: use that aligner")

    def trace_pairs(self, pair_queries, pair_subjects, cigar_cap=None, subject_base: int = 0, into=None, workspace_bytes=None):
        """Score, aligned span and canonical edit script of every pair (pair_queries[p], pair_subjects[p]) against the
        resident bucket, under THIS aligner's scoring (self.params()): BitPAl with any score set, global or semi-global,
        Myers semi-global, and Myers global (there a cross-check of align_pairs from another kernel).  Returns
        (score[n] int32 — as score() reports the pair —, span[n, 4] int32 = (q_begin, q_end, s_begin, s_end) half-open,
        n_ops[n] int32, cigar[n, cap] runs `length << 4 | BAM op` held as int32) device tensors; the runs cover the aligned
        span only.  Subject ids, subject_base, into= (the quadruple of an earlier call), cigar_cap and workspace_bytes are
        as in align_pairs; fresh outputs hold score 0, span -1, n_ops 0 and cigar 0 for pairs nobody owns.  The banded
        filter and Myers +distance raise (rc=-2) before any launch or allocation."""
        torch = self.torch
        self._trace_refusals("trace_pairs")
        pq = torch.as_tensor(pair_queries).to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        ps = torch.as_tensor(pair_subjects).to(device=self.device, dtype=torch.int64).contiguous().reshape(-1)
        if pq.numel() != ps.numel():
            raise BgsaHipError("trace_pairs: pair_queries and pair_subjects differ in length")
        n = pq.numel()
        cap = self.qlen + self.slen if cigar_cap is None else int(cigar_cap)
        if cap < 1:
            raise BgsaHipError("trace_pairs: rc=-1: cigar_cap is not positive")
        shapes = [((n,), torch.int32), ((n, 4), torch.int32), ((n,), torch.int32), ((n, cap), torch.int32)]
        if into is None:
            score, span, n_ops, cigar = (torch.full(shape, fill, dtype=dtype, device=self.device)
                                         for (shape, dtype), fill in zip(shapes, (0, -1, 0, 0)))
        else:
            (score, span, n_ops, cigar), _ = self._hit_lists(into, shapes, "trace_pairs")
        if n == 0:
            return score, span, n_ops, cigar
        if workspace_bytes is None:
            workspace_bytes = int(lib().bgsa_hip_align_pairs_workspace_bytes(self.qlen, self.slen, n))
        work, work_bytes = None, 0
        if workspace_bytes:
            if getattr(self, "d_align_work", None) is None or self.d_align_work.numel() < workspace_bytes:
                self.d_align_work = torch.empty(int(workspace_bytes), dtype=torch.uint8, device=self.device)
            work, work_bytes = self.d_align_work.data_ptr(), int(workspace_bytes)
        p = self.params()
        if self.d_lens is not None and self.reads_ragged:
            check(lib().bgsa_hip_myers_place_trace_pairs_lens_dev(self.d_content.data_ptr(), self.d_peq.data_ptr(), self.d_lens.data_ptr(),
                                                                  self.qlen, self.slen, self.ns, self.wn, pq.data_ptr(), ps.data_ptr(), n,
                                                                  self.nq, int(subject_base), score.data_ptr(), span.data_ptr(),
                                                                  n_ops.data_ptr(), cigar.data_ptr(), cap, work, work_bytes,
                                                                  self._stream()), "myers_place_trace_pairs_lens_dev")
            return score, span, n_ops, cigar
        if self.d_lens is not None:
            check(lib().bgsa_hip_trace_pairs_lens_dev(ctypes.byref(p), self.d_content.data_ptr(), self.d_peq.data_ptr(),
                                                      self.d_lens.data_ptr(), self.qlen, self.slen, self.ns, self.wn, pq.data_ptr(),
                                                      ps.data_ptr(), n, self.nq, int(subject_base), score.data_ptr(), span.data_ptr(),
                                                      n_ops.data_ptr(), cigar.data_ptr(), cap, work, work_bytes, self._stream()),
                  "trace_pairs_lens_dev")
            return score, span, n_ops, cigar
        check(lib().bgsa_hip_trace_pairs_dev(ctypes.byref(p), self.d_content.data_ptr(), self.d_peq.data_ptr(), self.qlen, self.slen,
                                             self.ns, self.wn, pq.data_ptr(), ps.data_ptr(), n, self.nq, int(subject_base),
                                             score.data_ptr(), span.data_ptr(), n_ops.data_ptr(), cigar.data_ptr(), cap, work, work_bytes,
                                             self._stream()), "trace_pairs_dev")
        return score, span, n_ops, cigar

    def trace_hits(self, hit_subjects, cigar_cap=None, subject_base: int = 0, into=None, workspace_bytes=None):
        """trace_pairs for the subjects[nq, K] tensor of top_hits / threshold_hits: row q holds subjects of query q.  Returns
        (score[nq, K], span[nq, K, 4], n_ops[nq, K], cigar[nq, K, cap]); unused slots (subject -1) keep score 0, span -1,
        n_ops 0.  into= the quadruple of an earlier call, for walking buckets."""
        torch = self.torch
        self._trace_refusals("trace_hits")
        hs = torch.as_tensor(hit_subjects).to(device=self.device, dtype=torch.int64)
        if hs.dim() != 2 or hs.shape[0] != self.nq:
            raise BgsaHipError(f"trace_hits: hit_subjects must be [nq = {self.nq}, K]")
        nq, k = hs.shape
        pq = torch.arange(nq, dtype=torch.int32, device=self.device).repeat_interleave(k)
        if into is not None:
            into = list(into)
            if len(into) != 4 or any(not t.is_contiguous() for t in into) or tuple(into[0].shape) != (nq, k) or \
                    tuple(into[1].shape) != (nq, k, 4) or tuple(into[2].shape) != (nq, k) or into[3].dim() != 3 or \
                    tuple(into[3].shape[:2]) != (nq, k):
                raise BgsaHipError(f"trace_hits: into= needs contiguous tensors of shape ({nq}, {k}), ({nq}, {k}, 4), ({nq}, {k}), ({nq}, {k}, cap)")
            if cigar_cap is None:
                cigar_cap = into[3].shape[2]
            into = (into[0].view(-1), into[1].view(nq * k, 4), into[2].view(-1), into[3].view(nq * k, -1))
        score, span, n_ops, cigar = self.trace_pairs(pq, hs.contiguous().view(-1), cigar_cap, subject_base, into, workspace_bytes)
        return score.view(nq, k), span.view(nq, k, 4), n_ops.view(nq, k), cigar.view(nq, k, -1)

    # ---- the Myers semi-global placement within a distance bound, reads of any length (bgsa_hip_myers_place_pairs_banded_dev) ----
    def place_pairs_banded(self, pair_queries, pair_subjects, max_distance: int, cigar_cap=None, subject_base: int = 0, into=None,
                           workspace_bytes=None):
        """trace_pairs for the Myers semi-global aligner with the history limited to the band of max_distance: reads of any
        length the scoring call takes.  Returns (distance[n] int32 = minus the score score() reports, exact whatever the bound,
        span[n, 4] int32 = (q_begin, q_end, 0, slen), n_ops[n] int32, cigar[n, cap]) device tensors.  A pair whose distance is
        <= min(max_distance, slen) gets exactly trace_pairs' span, n_ops and runs; any other owned pair keeps its exact distance
        and q_end and gets q_begin -1, n_ops 0 and an untouched cigar row.  Subject ids, subject_base, into= (the quadruple of an
        earlier call), cigar_cap and workspace_bytes are as in align_pairs_banded; fresh outputs hold distance -1, span -1,
        n_ops 0 and cigar 0 for pairs nobody owns.  Only ALGO_MYERS with semi_global=True (not +distance), one read length per
        bucket: anything else raises rc=-2 before any launch."""
        torch = self.torch
        if self.algo != ALGO_MYERS or not self.semi_global or self.scores == (0, 1, 1):
            raise BgsaHipError("place_pairs_banded: rc=-2: only the Myers unit-cost semi-global aligner places reads (no global mode "
                               "— align_pairs_banded —, no BitPAl score sets, no banded filter; +distance aligns the same as "
                               "-distance: use that aligner)")
        if self.d_lens is not None:
            raise BgsaHipError("place_pairs_banded: rc=-2: a bucket of mixed read lengths has no band-limited variant (one window "
                               "schedule per read length)")
        max_distance = min(int(max_distance), 2 ** 31 - 1)
        if max_distance < 0:
            raise BgsaHipError("place_pairs_banded: rc=-1: max_distance is negative")
        pq = torch.as_tensor(pair_queries).to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        ps = torch.as_tensor(pair_subjects).to(device=self.device, dtype=torch.int64).contiguous().reshape(-1)
        if pq.numel() != ps.numel():
            raise BgsaHipError("place_pairs_banded: pair_queries and pair_subjects differ in length")
        n = pq.numel()
        cap = self.qlen + self.slen if cigar_cap is None else int(cigar_cap)
        if cap < 1:
            raise BgsaHipError("place_pairs_banded: rc=-1: cigar_cap is not positive")
        shapes = [((n,), torch.int32), ((n, 4), torch.int32), ((n,), torch.int32), ((n, cap), torch.int32)]
        if into is None:
            distance, span, n_ops, cigar = (torch.full(shape, fill, dtype=dtype, device=self.device)
                                            for (shape, dtype), fill in zip(shapes, (-1, -1, 0, 0)))
        else:
            (distance, span, n_ops, cigar), _ = self._hit_lists(into, shapes, "place_pairs_banded")
        if n == 0:
            return distance, span, n_ops, cigar

        def call(n_pairs, work, work_bytes):
            check(lib().bgsa_hip_myers_place_pairs_banded_dev(self.d_content.data_ptr(), self.d_peq.data_ptr(), self.qlen, self.slen, self.ns,
                                                              self.wn, pq.data_ptr(), ps.data_ptr(), n_pairs, self.nq, int(subject_base),
                                                              max_distance, distance.data_ptr(), span.data_ptr(), n_ops.data_ptr(),
                                                              cigar.data_ptr(), cap, work, work_bytes, self._stream()),
                  "myers_place_pairs_banded_dev")
        if workspace_bytes is None:
            call(0, None, 0)   # an empty list runs the C call's checks alone: a window too wide is refused before a workspace is allocated for it
            workspace_bytes = int(lib().bgsa_hip_place_pairs_banded_workspace_bytes(self.qlen, self.slen, max_distance, n))
        call(n, *self._align_workspace(workspace_bytes))
        return distance, span, n_ops, cigar

    def place_hits_banded(self, hit_subjects, max_distance: int, cigar_cap=None, subject_base: int = 0, into=None, workspace_bytes=None):
        """place_pairs_banded for the subjects[nq, K] tensor of top_hits / threshold_hits, as trace_hits is for trace_pairs:
        (distance[nq, K], span[nq, K, 4], n_ops[nq, K], cigar[nq, K, cap]); unused slots (subject -1) keep distance -1, span -1,
        n_ops 0.  into= the quadruple of an earlier call, for walking buckets."""
        torch = self.torch
        hs = torch.as_tensor(hit_subjects).to(device=self.device, dtype=torch.int64)
        if hs.dim() != 2 or hs.shape[0] != self.nq:
            raise BgsaHipError(f"place_hits_banded: hit_subjects must be [nq = {self.nq}, K]")
        nq, k = hs.shape
        pq = torch.arange(nq, dtype=torch.int32, device=self.device).repeat_interleave(k)
        if into is not None:
            into = list(into)
            if len(into) != 4 or any(not t.is_contiguous() for t in into) or tuple(into[0].shape) != (nq, k) or \
                    tuple(into[1].shape) != (nq, k, 4) or tuple(into[2].shape) != (nq, k) or into[3].dim() != 3 or \
                    tuple(into[3].shape[:2]) != (nq, k):
                raise BgsaHipError(f"place_hits_banded: into= needs contiguous tensors of shape ({nq}, {k}), ({nq}, {k}, 4), ({nq}, {k}), ({nq}, {k}, cap)")
            if cigar_cap is None:
                cigar_cap = into[3].shape[2]
            into = (into[0].view(-1), into[1].view(nq * k, 4), into[2].view(-1), into[3].view(nq * k, -1))
        distance, span, n_ops, cigar = self.place_pairs_banded(pq, hs.contiguous().view(-1), max_distance, cigar_cap, subject_base, into,
                                                               workspace_bytes)
        return distance.view(nq, k), span.view(nq, k, 4), n_ops.view(nq, k), cigar.view(nq, k, -1)

    def check_faults(self) -> None:
        """Synchronises and raises if a kernel reported a stream fault (bgsa_hip_stream_faults)."""
        self.torch.cuda.synchronize(self.device)
        flags = int(lib().bgsa_hip_stream_faults(1))
        if flags:
            raise BgsaHipError(f"stream fault: {lib().bgsa_hip_last_error().decode()}")

    def _select(self) -> None:
        # the process-global selection of the C ABI (the reference's ints), for the entry points that read it
        if self.algo == ALGO_BITPAL:
            check(lib().bgsa_hip_select_scores(*(self.scores or (2, -3, -5))), "select_scores")
        elif self.algo == ALGO_MYERS and self.scores == (0, 1, 1):
            check(lib().bgsa_hip_select_scores(0, 1, 1), "select_scores")       # generator -m 1: +distance
        else:   # also resets the score ints a BitPAl / +distance selection left behind
            check(lib().bgsa_hip_select_algorithm(self.algo), "select_algorithm")
        check(lib().bgsa_hip_select_alignment(1 if self.semi_global else 0), "select_alignment")

    def kernel_name(self) -> str:
        self._select()
        name = lib().bgsa_hip_kernel_name(self.algo, self.wn).decode()
        lib().bgsa_hip_select_alignment(0)
        return name


def align_all_pairs(queries: np.ndarray, subjects: np.ndarray, algo: int = ALGO_MYERS, k: int = 0,
                    device: str = "cuda:0", scores=None, semi_global: bool = False) -> np.ndarray:
    """Convenience: scores[nq, ns] for small inputs, through the device-resident C ABI."""
    a = DeviceAligner(algo, device, k, scores, semi_global)
    a.set_queries(queries)
    a.set_subjects(subjects)
    out = a.score()
    a.check_faults()
    return out[:, : a.ns_real].cpu().numpy()


def align_all_pairs_ragged(queries: np.ndarray, subjects, algo: int = ALGO_MYERS, scores=None, device: str = "cuda:0") -> np.ndarray:
    """scores[nq, ns] of queries (ONE length: group queries by length) against subjects of mixed lengths (byte strings or 1-D
    uint8 arrays), columns in the caller's order.  Global modes (DeviceAligner.set_subjects_ragged).  The subjects are binned by
    the words they occupy (bin_by_words) and every bin is one bucket of its own longest read, so a short read is not scored at
    the width of the longest."""
    seqs = list(subjects)
    lens = pad_ragged(seqs)[1]
    a = DeviceAligner(algo, device, 0, scores)
    a.set_queries(queries)
    out = np.empty((a.nq, len(seqs)), dtype=np.int16)
    for idx in bin_by_words(lens):
        a.set_subjects_ragged([seqs[i] for i in idx])
        out[:, idx] = a.score()[:, : a.ns_real].cpu().numpy()
    a.check_faults()
    return out


def align_top_hits_ragged(queries: np.ndarray, subjects, k_best: int, algo: int = ALGO_MYERS, scores=None, device: str = "cuda:0",
                          smallest=None, block_rows: int = 1000) -> tuple[np.ndarray, np.ndarray]:
    """The k_best best subjects per query as (scores[nq, K] int32, subjects[nq, K] int64 — the caller's indices, -1 in an unused
    slot) over subjects of mixed lengths, binned as in align_all_pairs_ragged: the bins are walked with top_hits(into=,
    subject_base=) and the reported ids are mapped back to the caller's indices on the host.  Ties between equal scores go to
    the earlier position in the BINNED order (ascending word count, the caller's order within a bin), not to the smaller caller
    index.  Queries keep one length per call."""
    seqs = list(subjects)
    lens = pad_ragged(seqs)[1]
    bins = bin_by_words(lens)
    order = np.concatenate(bins)
    a = DeviceAligner(algo, device, 0, scores)
    a.set_queries(queries)
    into, base = None, 0
    for idx in bins:
        a.set_subjects_ragged([seqs[i] for i in idx])
        into = a.top_hits(k_best, block_rows=block_rows, smallest=smallest, subject_base=base, into=into)
        base += len(idx)
    a.check_faults()
    hit_scores, ids = into[0].cpu().numpy(), into[1].cpu().numpy()
    return hit_scores, np.where(ids >= 0, order[np.clip(ids, 0, order.size - 1)], -1)


CIGAR_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}   # the BAM op codes bgsa_hip_myers_align_pairs_dev / bgsa_hip_trace_pairs_dev write


def cigar_strings(n_ops, cigar) -> list[str]:
    """Host helper: the runs of align_pairs / align_hits / trace_pairs / trace_hits as text, e.g. "97=1X30=2D22=" — one string per pair in row-major
    order of the leading dimensions ("" for a pair with no runs: an unused slot).  Raises if a row overflowed its cap."""
    def host(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    counts = host(n_ops).reshape(-1)
    runs = host(cigar)
    runs = np.ascontiguousarray(runs).view(np.uint32).reshape(counts.size, -1) if counts.size else np.zeros((0, 1), np.uint32)
    cap = runs.shape[1]
    out = []
    for p, n in enumerate(counts.tolist()):
        if n > cap:
            raise BgsaHipError(f"cigar_strings: pair {p} has {n} runs, its row holds {cap} (raise cigar_cap)")
        out.append("".join(f"{w >> 4}{CIGAR_OPS[w & 15]}" for w in runs[p, :n].tolist()))
    return out


def align_top_alignments(queries: np.ndarray, subjects: np.ndarray, k_best: int, device: str = "cuda:0", block_rows: int = 1000,
                         cigar_cap=None):
    """Convenience beside align_top_hits (Myers global): the k_best best subjects per query AND their alignments, as
    (scores[nq, K] int32, subjects[nq, K] int64, cigars) with cigars[q][r] the edit script of query q against its r-th hit
    as a string, or None for an unused slot.  Selected and traced back on the device."""
    a = DeviceAligner(ALGO_MYERS, device)
    a.set_queries(queries)
    a.set_subjects(subjects)
    hit_scores, hit_subjects = a.top_hits(k_best, block_rows=block_rows)
    _, n_ops, cigar = a.align_hits(hit_subjects, cigar_cap=cigar_cap)
    a.check_faults()
    subj = hit_subjects.cpu().numpy()
    text = cigar_strings(n_ops, cigar)
    k = subj.shape[1]
    cigars = [[text[q * k + r] if subj[q, r] >= 0 else None for r in range(k)] for q in range(subj.shape[0])]
    return hit_scores.cpu().numpy(), subj, cigars


def align_top_alignments_banded(queries: np.ndarray, subjects: np.ndarray, k_best: int, max_distance=None, device: str = "cuda:0",
                                block_rows: int = 1000, cigar_cap=None):
    """align_top_alignments for subjects of any length: the k_best best subjects per query and their alignments within
    max_distance, as (scores[nq, K] int32, subjects[nq, K] int64, cigars); cigars[q][r] is None for an unused slot and for
    a hit beyond max_distance.  max_distance=None: the worst distance in the hit lists, so that every hit is aligned —
    one scalar read back from the device, the only synchronisation before the results are copied out."""
    a = DeviceAligner(ALGO_MYERS, device)
    a.set_queries(queries)
    a.set_subjects(subjects)
    hit_scores, hit_subjects = a.top_hits(k_best, block_rows=block_rows)
    if max_distance is None:
        max_distance = -int(a.torch.where(hit_subjects >= 0, hit_scores, a.torch.zeros_like(hit_scores)).min().item())
    distance, n_ops, cigar = a.align_hits_banded(hit_subjects, max_distance, cigar_cap=cigar_cap)
    a.check_faults()
    subj, dist = hit_subjects.cpu().numpy(), distance.cpu().numpy()
    text = cigar_strings(n_ops, cigar)
    k = subj.shape[1]
    cigars = [[text[q * k + r] if subj[q, r] >= 0 and dist[q, r] >= 0 else None for r in range(k)] for q in range(subj.shape[0])]
    return hit_scores.cpu().numpy(), subj, cigars


def trace_top_hits(queries: np.ndarray, subjects: np.ndarray, k_best: int, algo: int, scores=None,
                   semi_global: bool = False, k: int = 0, device: str = "cuda:0", block_rows: int = 1000, cigar_cap=None):
    """The counterpart of align_top_alignments for the other aligners (BitPAl score sets, the semi-global modes): the
    k_best best subjects per query AND where and how they align, as (scores[nq, K] int32, subjects[nq, K] int64,
    spans[nq, K, 4] int32 = (q_begin, q_end, s_begin, s_end), cigars) with cigars[q][r] the edit script of the aligned span
    as a string, or None for an unused slot (its span is -1).  Selected and traced back on the device."""
    a = DeviceAligner(algo, device, k, scores, semi_global)
    a.set_queries(queries)
    a.set_subjects(subjects)
    hit_scores, hit_subjects = a.top_hits(k_best, block_rows=block_rows)
    _, span, n_ops, cigar = a.trace_hits(hit_subjects, cigar_cap=cigar_cap)
    a.check_faults()
    subj = hit_subjects.cpu().numpy()
    text = cigar_strings(n_ops, cigar)
    kk = subj.shape[1]
    cigars = [[text[q * kk + r] if subj[q, r] >= 0 else None for r in range(kk)] for q in range(subj.shape[0])]
    return hit_scores.cpu().numpy(), subj, span.cpu().numpy(), cigars


def align_top_hits(queries: np.ndarray, subjects: np.ndarray, k_best: int, algo: int = ALGO_MYERS, k: int = 0,
                   device: str = "cuda:0", scores=None, semi_global: bool = False, smallest=None,
                   block_rows: int = 1000) -> tuple[np.ndarray, np.ndarray]:
    """Convenience: the k_best best subjects per query as (scores[nq, K] int32, subjects[nq, K] int64), selected on the
    device block by block — the [nq, ns] score matrix is never built (DeviceAligner.top_hits)."""
    a = DeviceAligner(algo, device, k, scores, semi_global)
    a.set_queries(queries)
    a.set_subjects(subjects)
    hit_scores, hit_subjects = a.top_hits(k_best, block_rows=block_rows, smallest=smallest)
    a.check_faults()
    return hit_scores.cpu().numpy(), hit_subjects.cpu().numpy()


def align_top_queries(queries: np.ndarray, subjects: np.ndarray, k_best: int, algo: int = ALGO_MYERS, k: int = 0,
                      device: str = "cuda:0", scores=None, semi_global: bool = False, smallest=None,
                      block_rows: int = 1000) -> tuple[np.ndarray, np.ndarray]:
    """Convenience: the k_best best queries per SUBJECT as (scores[ns, K] int32, queries[ns, K] int32), selected on the
    device block by block — the [nq, ns] score matrix is never built (DeviceAligner.top_queries)."""
    a = DeviceAligner(algo, device, k, scores, semi_global)
    a.set_queries(queries)
    a.set_subjects(subjects)
    hit_scores, hit_queries = a.top_queries(k_best, block_rows=block_rows, smallest=smallest)
    a.check_faults()
    return hit_scores.cpu().numpy(), hit_queries.cpu().numpy()


def align_top_queries_ragged(queries: np.ndarray, subjects, k_best: int, algo: int = ALGO_MYERS, scores=None, device: str = "cuda:0",
                             smallest=None, block_rows: int = 1000) -> tuple[np.ndarray, np.ndarray]:
    """The k_best best queries per subject as (scores[ns, K] int32, queries[ns, K] int32) over subjects of mixed lengths, rows
    in the caller's subject order.  The subjects are binned as in align_all_pairs_ragged; a bin's lists belong to its own
    subjects, so they are scattered to the caller's positions and nothing is merged: the ids are query ids and ties go to the
    smaller one, whatever the binning.  Queries keep one length per call."""
    seqs = list(subjects)
    lens = pad_ragged(seqs)[1]
    a = DeviceAligner(algo, device, 0, scores)
    a.set_queries(queries)
    k_best = int(k_best)
    out_scores = np.empty((len(seqs), k_best), dtype=np.int32)
    out_queries = np.empty((len(seqs), k_best), dtype=np.int32)
    for idx in bin_by_words(lens):
        a.set_subjects_ragged([seqs[i] for i in idx])
        hit_scores, hit_queries = a.top_queries(k_best, block_rows=block_rows, smallest=smallest)
        out_scores[idx] = hit_scores.cpu().numpy()
        out_queries[idx] = hit_queries.cpu().numpy()
    a.check_faults()
    return out_scores, out_queries


def trace_top_queries(queries: np.ndarray, subjects: np.ndarray, k_best: int, algo: int, scores=None,
                      semi_global: bool = False, k: int = 0, device: str = "cuda:0", block_rows: int = 1000, cigar_cap=None):
    """The counterpart of trace_top_hits per SUBJECT: the k_best best queries of every subject AND where and how they align, as
    (scores[ns, K] int32, queries[ns, K] int32, spans[ns, K, 4] int32 = (q_begin, q_end, s_begin, s_end), cigars) with
    cigars[c][r] the edit script of the aligned span as a string, or None for an unused slot (its span is -1).  Selected and
    traced back on the device (top_queries, query_hits_as_pairs, trace_pairs).  With ALGO_MYERS and semi_global=True this is
    read placement: windows of a reference as queries, reads as subjects — every read's best windows, the read's begin and end
    inside the window and its edit script."""
    a = DeviceAligner(algo, device, k, scores, semi_global)
    a.set_queries(queries)
    a.set_subjects(subjects)
    hit_scores, hit_queries = a.top_queries(k_best, block_rows=block_rows)
    pair_queries, pair_subjects = a.query_hits_as_pairs(hit_queries)
    _, span, n_ops, cigar = a.trace_pairs(pair_queries, pair_subjects, cigar_cap=cigar_cap)
    a.check_faults()
    ids = hit_queries.cpu().numpy()
    text = cigar_strings(n_ops, cigar)
    ns, kk = ids.shape
    cigars = [[text[c * kk + r] if ids[c, r] >= 0 else None for r in range(kk)] for c in range(ns)]
    return hit_scores.cpu().numpy(), ids, span.cpu().numpy().reshape(ns, kk, 4), cigars


def place_top_queries_banded(queries: np.ndarray, subjects: np.ndarray, k_best: int, max_distance=None, device: str = "cuda:0",
                             block_rows: int = 1000, cigar_cap=None):
    """Read placement for reads of any length, beside trace_top_queries (which stops at 1,024 bp): windows of a reference as
    queries, reads as subjects, Myers semi-global.  The k_best best windows of every read AND where and how the read aligns
    inside them, within max_distance, as (scores[ns, K] int32, queries[ns, K] int32, spans[ns, K, 4] int32 = (q_begin, q_end, 0,
    slen), cigars); cigars[c][r] is None for an unused slot (its span is -1) and for a hit beyond max_distance (its span keeps
    q_begin -1).  max_distance=None: the worst distance in the hit lists, so that every hit is placed — one scalar read back
    from the device.  Selected, located and traced back on the device (top_queries, query_hits_as_pairs, place_pairs_banded)."""
    a = DeviceAligner(ALGO_MYERS, device, semi_global=True)
    a.set_queries(queries)
    a.set_subjects(subjects)
    hit_scores, hit_queries = a.top_queries(k_best, block_rows=block_rows)
    if max_distance is None:
        max_distance = -int(a.torch.where(hit_queries >= 0, hit_scores, a.torch.zeros_like(hit_scores)).min().item())
    pair_queries, pair_subjects = a.query_hits_as_pairs(hit_queries)
    _, span, n_ops, cigar = a.place_pairs_banded(pair_queries, pair_subjects, max_distance, cigar_cap=cigar_cap)
    a.check_faults()
    ids = hit_queries.cpu().numpy()
    ns, kk = ids.shape
    spans = span.cpu().numpy().reshape(ns, kk, 4)
    text = cigar_strings(n_ops, cigar)
    cigars = [[text[c * kk + r] if ids[c, r] >= 0 and spans[c, r, 0] >= 0 else None for r in range(kk)] for c in range(ns)]
    return hit_scores.cpu().numpy(), ids, spans, cigars


# reads mapped onto one reference: windows cut on the device, both strands, reference coordinates (bgsa_amd/reference.py)
from .reference import (ContigHits, ContigMapper, ContigPlacement, PairedHits, Placement, ReferenceHits, ReferenceMapper, SamRecords, blank_beyond, check_sam_call,  # noqa: E402
                        list_mapq, max_stride, rescue_region, rescue_slots, seed_plan, seed_plan_ragged, window_plan, write_sam, contig_layout, read_fasta,
                        BGZF_EOF, BamRecords, bgzf_blocks, check_bam_call, write_bam, BamIndex, SortedBamRecords, bai_bytes, check_mark_duplicates,
                        DUPLICATE_FLAG, DUPLICATE_MIN_QUALITY, DUPLICATE_STATS, BamMerge, check_bam_merge, check_bam_merge_add,
                        PILEUP_COLUMNS, PILEUP_EXCLUDE_FLAGS, PILEUP_STATS, Pileup, PileupSites, check_pileup, check_pileup_add, check_pileup_sites)
