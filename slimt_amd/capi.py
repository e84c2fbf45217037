"""ctypes binding of include/slimt_hip.h (slimt_amd/lib/libslimt_hip.so).

Thin: numpy arrays in/out, every call goes through the C ABI exactly as a
cgo/JNI/C++ host would. There is no fallback: if the library is missing or a
call fails, SlimtHipError is raised.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
from typing import Optional, Sequence

import numpy as np

from . import build as _build

MAX_ALTERNATIVES = 8  # SLIMT_HIP_MAX_ALTERNATIVES
CANDIDATE_RUN = 2  # SLIMT_HIP_CANDIDATE_RUN: consecutive candidates one attention workgroup walks (score_candidates.hip)

SYMBOLS = [
    "slimt_hip_abi_version", "slimt_hip_last_error", "slimt_hip_device_count",
    "slimt_hip_set_device", "slimt_hip_affine", "slimt_hip_affine_select",
    "slimt_hip_affine_acc_i32", "slimt_hip_prepare_weight_transposed",
    "slimt_hip_prepare_weight_quantized_transposed", "slimt_hip_layer_norm",
    "slimt_hip_softmax", "slimt_hip_highway", "slimt_hip_sdpa",
    "slimt_hip_request_hw_queues", "slimt_hip_hw_queues", "slimt_hip_model_create_from_bin",
    "slimt_hip_model_create", "slimt_hip_model_destroy", "slimt_hip_model_info",
    "slimt_hip_ctx_create", "slimt_hip_ctx_create_budget", "slimt_hip_ctx_destroy", "slimt_hip_contexts_on_device", "slimt_hip_ctx_stream",
    "slimt_hip_ctx_synchronize", "slimt_hip_ctx_set_decode_mode", "slimt_hip_ctx_set_encode_rows", "slimt_hip_ctx_plan", "slimt_hip_translate", "slimt_hip_translate_device",
    "slimt_hip_encode", "slimt_hip_decode_begin", "slimt_hip_decode_step",
    "slimt_hip_profile_enable", "slimt_hip_profile_read", "slimt_hip_profile_reset",
    "slimt_hip_debug_decode_stamps", "slimt_hip_debug_kv_formats", "slimt_hip_debug_kv_narrow_limit", "slimt_hip_debug_kv_tight_limit", "slimt_hip_debug_out_tied_exact", "slimt_hip_debug_tied_output_proof", "slimt_hip_debug_fused_decode_lds_bytes", "slimt_hip_debug_kv_tight_watch", "slimt_hip_debug_kv_centres", "slimt_hip_model_set_kv_centres", "slimt_hip_debug_kv_watch", "slimt_hip_debug_break_shortlist_handoff", "slimt_hip_debug_cross_attention",
    "slimt_hip_debug_occupancy_trace", "slimt_hip_debug_decoder_plan", "slimt_hip_model_set_decoder_budget",
    "slimt_hip_model_set_kv_cache_policy",
    "slimt_hip_model_set_xcd_affinity", "slimt_hip_model_device",
    "slimt_hip_model_set_kv_cache_format", "slimt_hip_model_set_adaptive_decoder_rows",
    "slimt_hip_shortlist_create", "slimt_hip_shortlist_destroy", "slimt_hip_shortlist_info",
    "slimt_hip_shortlist_generate", "slimt_hip_shortlist_generate_device",
    "slimt_hip_translate_device_generated", "slimt_hip_translate_generated", "slimt_hip_translate_async_generated",
    "slimt_hip_translate_async", "slimt_hip_host_alloc", "slimt_hip_host_free",
    "slimt_hip_encode_embedded", "slimt_hip_decode_begin_from", "slimt_hip_decode_step_states",
    "slimt_hip_translate_many_rows", "slimt_hip_translate_many_device", "slimt_hip_translate_many_async",
    "slimt_hip_debug_kv_recalibrations", "slimt_hip_translate_many_device_generated", "slimt_hip_translate_many_async_generated",
    "slimt_hip_ctx_set_scores", "slimt_hip_ctx_set_target_prefix", "slimt_hip_ctx_set_sampling", "slimt_hip_sampling_key",
    "slimt_hip_ctx_set_sampling_truncation", "slimt_hip_sample_truncated",
    "slimt_hip_score", "slimt_hip_score_async", "slimt_hip_score_device", "slimt_hip_score_async_generated",
    "slimt_hip_ctx_set_score_alternatives", "slimt_hip_debug_ctx_shortlists", "slimt_hip_debug_ctx_set_counters",
    "slimt_hip_score_candidates", "slimt_hip_score_candidates_async", "slimt_hip_score_candidates_device",
    "slimt_hip_score_candidates_async_generated", "slimt_hip_candidates_rank", "slimt_hip_candidates_rank_device",
    "slimt_hip_translate_fanout", "slimt_hip_translate_fanout_async", "slimt_hip_translate_fanout_device",
    "slimt_hip_translate_fanout_async_generated",
    "slimt_hip_consensus_select", "slimt_hip_consensus_select_device", "slimt_hip_ctx_set_fanout_consensus",
    "slimt_hip_translate_beam", "slimt_hip_translate_beam_async", "slimt_hip_translate_beam_device",
    "slimt_hip_translate_beam_async_generated", "slimt_hip_beam_step",
]

K_NONE, K_GEMM_ENC, K_GEMM_DEC, K_LOGITS, K_ATTN_ENC, K_ATTN_DEC, K_SSRU, K_DECODE_FUSED, K_ENCODE_FUSED = range(9)
K_CONSENSUS = 9  # (consensus selection: slimt_hip_consensus_select_device and armed fan-out calls)
CONSENSUS_MAX_ORDER, CONSENSUS_MAX_BETA2, CONSENSUS_MAX_ROWS, CONSENSUS_MAX_T = 4, 16, 64, 256  # (include/slimt_hip.h)
NO_ROW = 0xFFFFFFFF  # best[b] of a source without a competing row
KERNEL_NAMES = {K_GEMM_ENC: "gemm_enc", K_GEMM_DEC: "gemm_dec", K_LOGITS: "logits_argmax",
                K_ATTN_ENC: "attn_enc", K_ATTN_DEC: "attn_dec", K_SSRU: "ssru"}


class SlimtHipError(RuntimeError):
    pass


class _Param(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_int32), ("rows", C.c_int32),
                ("cols", C.c_int32), ("data", C.c_void_p), ("bytes", C.c_uint64)]


class _Batch(C.Structure):
    """slimt_hip_batch (include/slimt_hip.h): one batch of a merged launch."""
    _fields_ = [("src_ids", C.c_void_p), ("lengths", C.c_void_p), ("B", C.c_size_t), ("S", C.c_size_t), ("shortlist", C.c_void_p),
                ("n_shortlist", C.c_size_t), ("out_ids", C.c_void_p), ("out_len", C.c_void_p), ("align", C.c_void_p)]


class _Dims(C.Structure):
    _fields_ = [("encoder_layers", C.c_int32), ("decoder_layers", C.c_int32),
                ("num_heads", C.c_int32)]


_lib = None


def library_path() -> str:
    return _build.LIB_PATH


def _elf_soname(path: str):
    """DT_SONAME of a 64-bit little-endian ELF shared object (None when it has none or is not one)."""
    import struct
    try:
        with open(path, "rb") as f:
            head = f.read(64)
            if len(head) < 64 or head[:4] != b"\x7fELF" or head[4] != 2 or head[5] != 1:
                return None
            e_shoff, = struct.unpack_from("<Q", head, 0x28)
            e_shentsize, e_shnum = struct.unpack_from("<HH", head, 0x3A)
            sections = []
            for i in range(e_shnum):
                f.seek(e_shoff + i * e_shentsize)
                sh = f.read(e_shentsize)
                sh_type, = struct.unpack_from("<I", sh, 4)
                sh_offset, sh_size, sh_link = struct.unpack_from("<QQI", sh, 0x18)
                sections.append((sh_type, sh_offset, sh_size, sh_link))
            for sh_type, off, size, link in sections:
                if sh_type != 6:  # SHT_DYNAMIC
                    continue
                f.seek(off)
                dyn = f.read(size)
                for j in range(0, len(dyn) - 15, 16):
                    tag, val = struct.unpack_from("<qQ", dyn, j)
                    if tag == 14:  # DT_SONAME: offset into the linked string table
                        f.seek(sections[link][1] + val)
                        return f.read(256).split(b"\0", 1)[0].decode()
                    if tag == 0:
                        break
    except (OSError, struct.error, IndexError, UnicodeDecodeError):
        return None
    return None


def mapped_hip_runtimes():
    """Paths of the libamdhip64 images this process has mapped (one, unless something loaded a second runtime)."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    except OSError:
        return []


HIP_RUNTIME_SONAME = "libamdhip64.so.7"  # what libslimt_hip.so NEEDs


def _preload_hip_runtime() -> None:
    """One HIP runtime per process, whatever the import order. libslimt_hip.so NEEDs `libamdhip64.so.7` by
    SONAME: the dynamic loader binds that to a copy the process has mapped already (PyTorch imported first: its
    bundled one), else to ROCm's through the RUNPATH. PyTorch's own libraries ask for theirs by FILE, so with
    ROCm's copy mapped first a later `import torch` maps a second runtime next to it (and finds no GPU). When no
    runtime is mapped yet and an installed PyTorch bundles one WITH THAT SONAME (a PyTorch built against another ROCm
    major would be a second runtime, the very thing this avoids), map that one now: a later `import torch` then finds
    its own file already loaded, and both sides share it. Nothing is imported, no HIP call is made.
    SLIMT_HIP_NO_PRELOAD=1 switches this off (processes that never import torch)."""
    if os.environ.get("SLIMT_HIP_NO_PRELOAD") == "1" or mapped_hip_runtimes():
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for d in (spec.submodule_search_locations or []) if spec else []:
        cand = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(cand) and _elf_soname(cand) == HIP_RUNTIME_SONAME:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            return


def lib():
    """Load libslimt_hip.so (must have been built: __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise SlimtHipError(
            f"{path} is missing: build it with `python -m slimt_amd.build` "
            "(there is no CPU fallback)")
    _preload_hip_runtime()
    L = C.CDLL(path)
    if os.environ.get("SLIMT_HIP_LIB"):
        # an alternative library (A/B of builds, tools/ab_lib.sh): an OLDER one may lack the newest entry points -- they
        # then fail when called, not when the library is loaded
        class _Tolerant:
            def __init__(self, lib_):
                object.__setattr__(self, "_l", lib_)

            def __getattr__(self, name):
                try:
                    return getattr(self._l, name)
                except AttributeError:
                    def missing(*a, **k):
                        raise SlimtHipError(f"{name} is not exported by {path}")
                    missing.argtypes = missing.restype = None
                    object.__setattr__(self, name, missing)
                    return missing
        L = _Tolerant(L)
    if len(mapped_hip_runtimes()) > 1:  # (someone mapped another copy by file name before or behind us)
        import warnings
        warnings.warn("two HIP runtimes are mapped in this process (%s): the GPU may be invisible to one of them"
                      % ", ".join(mapped_hip_runtimes()), RuntimeWarning, stacklevel=2)
    vp, f32, sz, i32, u32 = C.c_void_p, C.c_float, C.c_size_t, C.c_int, C.c_uint32
    L.slimt_hip_abi_version.restype = i32
    L.slimt_hip_last_error.restype = C.c_char_p
    L.slimt_hip_device_count.argtypes = [vp]
    L.slimt_hip_set_device.argtypes = [i32]
    L.slimt_hip_affine.argtypes = [vp, sz, sz, vp, sz, vp, f32, f32, vp]
    L.slimt_hip_affine_select.argtypes = [vp, sz, sz, vp, sz, vp, f32, f32, vp, sz, vp]
    L.slimt_hip_affine_acc_i32.argtypes = [vp, sz, sz, vp, sz, f32, vp]
    L.slimt_hip_prepare_weight_transposed.argtypes = [vp, vp, f32, sz, sz]
    L.slimt_hip_prepare_weight_quantized_transposed.argtypes = [vp, vp, sz, sz]
    L.slimt_hip_layer_norm.argtypes = [vp, vp, vp, f32, sz, sz, vp]
    L.slimt_hip_softmax.argtypes = [vp, sz, sz, vp]
    L.slimt_hip_highway.argtypes = [vp, vp, vp, sz, vp]
    L.slimt_hip_sdpa.argtypes = [vp, vp, vp, vp, sz, sz, sz, sz, sz, vp, vp]
    L.slimt_hip_model_create.argtypes = [vp, sz, vp, i32, vp]
    L.slimt_hip_model_create_from_bin.argtypes = [vp, sz, vp, i32, vp]
    L.slimt_hip_request_hw_queues.argtypes = [i32]
    L.slimt_hip_hw_queues.restype = i32
    L.slimt_hip_model_destroy.argtypes = [vp]
    L.slimt_hip_model_info.argtypes = [vp, vp, vp, vp, vp]
    L.slimt_hip_ctx_create.argtypes = [vp, sz, sz, vp, vp]
    L.slimt_hip_ctx_destroy.argtypes = [vp]
    L.slimt_hip_contexts_on_device.argtypes = [i32, vp]
    L.slimt_hip_ctx_stream.argtypes = [vp, vp]
    L.slimt_hip_ctx_synchronize.argtypes = [vp]
    L.slimt_hip_ctx_set_decode_mode.argtypes = [vp, i32]
    L.slimt_hip_ctx_set_encode_rows.argtypes = [vp, i32]
    L.slimt_hip_ctx_set_scores.argtypes = [vp, vp, sz]
    L.slimt_hip_ctx_set_target_prefix.argtypes = [vp, vp, vp, sz]
    L.slimt_hip_ctx_set_sampling.argtypes = [vp, f32, vp, sz]
    L.slimt_hip_sampling_key.argtypes = [C.c_uint64, C.c_uint64]
    L.slimt_hip_sampling_key.restype = C.c_uint64
    L.slimt_hip_ctx_set_sampling_truncation.argtypes = [vp, u32, f32]
    L.slimt_hip_sample_truncated.argtypes = [vp, sz, sz, vp, f32, u32, f32, vp, vp, vp, vp, vp, vp]
    L.slimt_hip_ctx_plan.argtypes = [vp, sz, vp, vp]
    L.slimt_hip_translate.argtypes = [vp, vp, vp, sz, sz, vp, sz, f32, u32, vp, vp, vp]
    L.slimt_hip_translate_async.argtypes = [vp, vp, vp, sz, sz, vp, sz, f32, u32, vp, vp, vp]
    L.slimt_hip_host_alloc.argtypes = [sz, vp]
    L.slimt_hip_host_free.argtypes = [vp]
    L.slimt_hip_translate_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, f32, u32, vp, vp, vp, i32]
    L.slimt_hip_encode.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
    L.slimt_hip_decode_begin.argtypes = [vp, vp, sz]
    L.slimt_hip_encode_embedded.argtypes = [vp, vp, vp, sz, sz, vp]
    L.slimt_hip_decode_begin_from.argtypes = [vp, vp, vp, sz, sz, vp, sz]
    L.slimt_hip_decode_step_states.argtypes = [vp, vp, vp, vp, vp, vp]
    L.slimt_hip_decode_step.argtypes = [vp, vp, vp, vp, vp]
    L.slimt_hip_profile_enable.argtypes = [vp, i32]
    L.slimt_hip_profile_read.argtypes = [vp, vp, vp, vp, vp]
    L.slimt_hip_profile_reset.argtypes = [vp]
    L.slimt_hip_debug_decode_stamps.argtypes = [vp, i32, vp, sz]
    L.slimt_hip_debug_occupancy_trace.argtypes = [vp, sz]
    L.slimt_hip_debug_kv_formats.argtypes = [vp, vp, sz, vp]
    L.slimt_hip_debug_decoder_plan.argtypes = [vp, vp]
    L.slimt_hip_debug_kv_narrow_limit.argtypes = [vp, i32]
    L.slimt_hip_debug_kv_watch.argtypes = [vp, vp, vp, vp]
    L.slimt_hip_debug_kv_tight_limit.argtypes = [vp, i32]
    L.slimt_hip_debug_kv_tight_watch.argtypes = [vp, vp, vp, vp]
    L.slimt_hip_debug_out_tied_exact.argtypes = [vp, vp]
    L.slimt_hip_debug_tied_output_proof.argtypes = [vp, sz, sz, f32, vp]
    L.slimt_hip_debug_fused_decode_lds_bytes.argtypes = [C.c_int] * 7 + [C.c_uint, vp, vp, vp]
    L.slimt_hip_debug_kv_recalibrations.argtypes = [vp, vp, i32]
    L.slimt_hip_debug_kv_centres.argtypes = [vp, vp, sz, vp]
    L.slimt_hip_model_set_kv_centres.argtypes = [vp, vp, sz]
    L.slimt_hip_debug_break_shortlist_handoff.argtypes = [vp, i32, u32]
    L.slimt_hip_debug_ctx_shortlists.argtypes = [vp, sz, vp, sz, vp]
    L.slimt_hip_debug_ctx_set_counters.argtypes = [vp, u32]
    L.slimt_hip_debug_cross_attention.argtypes = [vp, i32, i32, vp, vp, vp]
    L.slimt_hip_model_set_decoder_budget.argtypes = [vp, i32]
    L.slimt_hip_model_set_kv_cache_policy.argtypes = [vp, i32]
    L.slimt_hip_model_set_xcd_affinity.argtypes = [vp, i32]
    L.slimt_hip_model_set_kv_cache_format.argtypes = [vp, i32]
    L.slimt_hip_model_set_adaptive_decoder_rows.argtypes = [vp, i32]
    L.slimt_hip_ctx_create_budget.argtypes = [vp, sz, sz, sz, vp, vp]
    L.slimt_hip_shortlist_create.argtypes = [vp, sz, sz, sz, i32, i32, i32, vp]
    L.slimt_hip_shortlist_destroy.argtypes = [vp]
    L.slimt_hip_shortlist_info.argtypes = [vp, vp, vp]
    L.slimt_hip_shortlist_generate.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    L.slimt_hip_shortlist_generate_device.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp]
    L.slimt_hip_translate_device_generated.argtypes = [vp, vp, vp, vp, sz, sz, f32, u32, vp, vp, vp, i32]
    L.slimt_hip_translate_generated.argtypes = [vp, vp, vp, vp, sz, sz, f32, u32, vp, vp, vp]
    L.slimt_hip_translate_async_generated.argtypes = [vp, vp, vp, vp, sz, sz, f32, u32, vp, vp, vp]
    L.slimt_hip_translate_many_rows.argtypes = [vp, sz]
    L.slimt_hip_translate_many_rows.restype = sz
    L.slimt_hip_translate_many_device.argtypes = [vp, vp, sz, sz, f32, u32, i32]
    L.slimt_hip_translate_many_async.argtypes = [vp, vp, sz, sz, f32, u32]
    L.slimt_hip_translate_many_device_generated.argtypes = [vp, vp, vp, sz, sz, f32, u32, i32]
    L.slimt_hip_translate_many_async_generated.argtypes = [vp, vp, vp, sz, sz, f32, u32]
    L.slimt_hip_score.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, vp]
    L.slimt_hip_score_async.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, vp]
    L.slimt_hip_score_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, vp]
    L.slimt_hip_score_async_generated.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, sz, vp, vp]
    L.slimt_hip_ctx_set_score_alternatives.argtypes = [vp, u32, vp, vp, vp]
    L.slimt_hip_score_candidates.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, sz, vp, vp]
    L.slimt_hip_score_candidates_async.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, sz, vp, vp]
    L.slimt_hip_score_candidates_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, sz, vp, vp]
    L.slimt_hip_score_candidates_async_generated.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, sz, vp, sz, vp, vp]
    L.slimt_hip_candidates_rank.argtypes = [vp, vp, vp, sz, sz, sz, i32, vp, vp]
    L.slimt_hip_candidates_rank_device.argtypes = [vp, vp, vp, vp, sz, sz, sz, i32, vp, vp]
    L.slimt_hip_translate_fanout.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, sz, f32, u32, vp, vp, vp]
    L.slimt_hip_translate_fanout_async.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, sz, f32, u32, vp, vp, vp]
    L.slimt_hip_translate_fanout_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, sz, f32, u32, vp, vp, vp, i32]
    L.slimt_hip_translate_fanout_async_generated.argtypes = [vp, vp, vp, vp, sz, sz, vp, sz, f32, u32, vp, vp, vp]
    L.slimt_hip_consensus_select.argtypes = [vp, vp, vp, sz, sz, sz, i32, i32, vp, vp]
    L.slimt_hip_consensus_select_device.argtypes = [vp, vp, vp, vp, sz, sz, sz, i32, i32, vp, vp]
    L.slimt_hip_ctx_set_fanout_consensus.argtypes = [vp, i32, i32, vp, vp]
    L.slimt_hip_translate_beam.argtypes = [vp, vp, vp, sz, sz, i32, i32, vp, sz, f32, u32, vp, vp, vp, vp, vp]
    L.slimt_hip_translate_beam_async.argtypes = [vp, vp, vp, sz, sz, i32, i32, vp, sz, f32, u32, vp, vp, vp, vp, vp]
    L.slimt_hip_translate_beam_device.argtypes = [vp, vp, vp, sz, sz, i32, i32, vp, sz, f32, u32, vp, vp, vp, vp, vp, i32]
    L.slimt_hip_translate_beam_async_generated.argtypes = [vp, vp, vp, vp, sz, sz, i32, i32, f32, u32, vp, vp, vp, vp, vp]
    L.slimt_hip_beam_step.argtypes = [vp, sz, i32, sz, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("slimt_hip_abi_version",):
            fn.restype = C.c_int
    _lib = L
    return L


def sampling_key(seed: int, index: int) -> int:
    """slimt_hip_sampling_key: the key of sentence `index` of a request seeded `seed`."""
    return int(lib().slimt_hip_sampling_key(int(seed) & (2 ** 64 - 1), int(index) & (2 ** 64 - 1)))


def sampling_keys(seed: int, n: int, first: int = 0) -> np.ndarray:
    """the keys of sentences first .. first + n - 1 of a request seeded `seed` (uint64 [n])"""
    return np.array([sampling_key(seed, first + i) for i in range(n)], dtype=np.uint64)


def sample_truncated(logits, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, ids=None, keys=None, steps=None):
    """slimt_hip_sample_truncated: one truncated sampled step over logits [M, N] (float32). ids: the columns' vocabulary
    ids (uint32 [N]; None: the column), keys: the rows' sentence keys (uint64 [M]; None: the row index), steps: the rows'
    step (uint32 [M]; None: 0). Returns (columns uint32 [M], thresholds float32 [M], kept uint32 [M], scores float32 [M])."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    M, N = logits.shape
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
    keys = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
    steps = None if steps is None else np.ascontiguousarray(steps, dtype=np.uint32)
    if (ids is not None and ids.shape != (N,)) or (keys is not None and keys.shape != (M,)) or (steps is not None and steps.shape != (M,)):
        raise ValueError("sample_truncated: ids [N], keys [M] and steps [M] expected")
    cols, thr = np.zeros(M, np.uint32), np.zeros(M, np.float32)
    kept, sc = np.zeros(M, np.uint32), np.zeros(M, np.float32)
    _chk(lib().slimt_hip_sample_truncated(_p(logits), M, N, _p(ids), float(temperature), int(top_k), float(top_p), _p(keys),
                                          _p(steps), _p(cols), _p(thr), _p(kept), _p(sc)))
    return cols, thr, kept, sc


MAX_BEAM = 8  # SLIMT_HIP_MAX_BEAM
BEAM_DEAD, BEAM_LIVE, BEAM_FINISHED = 0, 1, 2
BEAM_NONE = 0xFFFFFFFF


def beam_step(logits, totals, flags, beam: int, eos_id: int = 0, ids=None):
    """slimt_hip_beam_step: one selection of the beam search over logits [B * beam, N] (float32), the slots' totals
    [B * beam] float32 and flags [B * beam] uint32 (0 dead, 1 live, 2 finished). ids: the columns' vocabulary ids (uint32
    [N]; None: the column). Returns (parent, token, token_score, totals, flags), each [B * beam]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    totals = np.ascontiguousarray(totals, dtype=np.float32)
    flags = np.ascontiguousarray(flags, dtype=np.uint32)
    beam = int(beam)
    if logits.ndim != 2 or beam < 1 or logits.shape[0] % beam or totals.shape != (logits.shape[0],) or flags.shape != totals.shape:
        raise ValueError("beam_step: logits [B * beam, N], totals [B * beam] and flags [B * beam] expected")
    R, N = logits.shape
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
    if ids is not None and ids.shape != (N,):
        raise ValueError("beam_step: ids [N] expected")
    parent, token, flags_out = np.zeros(R, np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.uint32)
    score, totals_out = np.zeros(R, np.float32), np.zeros(R, np.float32)
    _chk(lib().slimt_hip_beam_step(_p(logits), R // beam, beam, N, _p(ids), _p(totals), _p(flags), int(eos_id), _p(parent),
                                   _p(token), _p(score), _p(totals_out), _p(flags_out)))
    return parent, token, score, totals_out, flags_out


def candidates_rank(scores, tgt_len, cand_src, B: int, mean: bool = False, mode=None):
    """slimt_hip_candidates_rank: scores [N, T] float32, tgt_len [N], cand_src [N] (< B). Returns (totals float32 [N] -- each
    candidate's f32 sum over t < tgt_len[c], ascending t from +0 -- and best uint32 [B] -- per source the lowest index among
    the candidates of the largest key, 0xFFFFFFFF where none competes; the key is the total, or with mean=True the total
    divided by the length). mode: the C call's integer, where that is what is tested (overrides mean)."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    tgt_len = np.ascontiguousarray(tgt_len, dtype=np.uint32)
    cand_src = np.ascontiguousarray(cand_src, dtype=np.uint32)
    if scores.ndim != 2 or tgt_len.shape != scores.shape[:1] or cand_src.shape != scores.shape[:1]:
        raise ValueError("candidates_rank: scores [N, T], tgt_len [N] and cand_src [N] expected, got %s, %s, %s"
                         % (scores.shape, tgt_len.shape, cand_src.shape))
    N, T = scores.shape
    totals, best = np.zeros(N, np.float32), np.zeros(int(B), np.uint32)
    _chk(lib().slimt_hip_candidates_rank(_p(scores), _p(tgt_len), _p(cand_src), N, T, int(B),
                                         int(bool(mean)) if mode is None else int(mode), _p(totals), _p(best)))
    return totals, best


def consensus_select(ids, lengths, row_src, B: int, max_order: int = 4, beta2: int = 4):
    """slimt_hip_consensus_select: ids [N, T] uint32, lengths [N], row_src [N] (< B). Returns (utility float64 [N] -- each
    row's mean token n-gram F (orders 1..max_order, integer beta2 = beta^2) against the other non-empty rows of its source --
    and best uint32 [B] -- per source the lowest row of the largest utility, NO_ROW where no row competes)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    row_src = np.ascontiguousarray(row_src, dtype=np.uint32)
    if ids.ndim != 2 or lengths.shape != ids.shape[:1] or row_src.shape != ids.shape[:1]:
        raise ValueError("consensus_select: ids [N, T], lengths [N] and row_src [N] expected, got %s, %s, %s"
                         % (ids.shape, lengths.shape, row_src.shape))
    N, T = ids.shape
    utility, best = np.zeros(N, np.float64), np.zeros(int(B), np.uint32)
    _chk(lib().slimt_hip_consensus_select(_p(ids), _p(lengths), _p(row_src), N, T, int(B), int(max_order), int(beta2),
                                          _p(utility), _p(best)))
    return utility, best


def translate_many_rows(sizes) -> int:
    """Global sentences a merged launch of these batch sizes occupies in its context (max_batch)."""
    a = (C.c_size_t * len(sizes))(*[int(x) for x in sizes])
    return int(lib().slimt_hip_translate_many_rows(a, len(sizes)))


def contexts_on_device(device: int = 0) -> int:
    """slimt_hip_contexts_on_device: contexts (streams) this process holds on `device`; past 22 the device's hardware
    queues are time-sliced and the library says so once on stderr."""
    n = C.c_int(0)
    if lib().slimt_hip_contexts_on_device(int(device), C.byref(n)):
        raise SlimtHipError(lib().slimt_hip_last_error().decode())
    return int(n.value)


def request_hw_queues(n: int = 32) -> bool:
    """slimt_hip_request_hw_queues: ask the HIP runtime for `n` hardware queues (GPU_MAX_HW_QUEUES, unless the
    process has set it) -- one per concurrent translate worker's stream; the default of four makes 20 workers
    take turns. Only before the library's first HIP call: returns False when it came too late."""
    rc = lib().slimt_hip_request_hw_queues(int(n))
    if rc < 0:
        raise SlimtHipError(lib().slimt_hip_last_error().decode())
    return rc == 0


def _chk(rc: int) -> None:
    if rc != 0:
        raise SlimtHipError(f"slimt_hip error {rc}: {lib().slimt_hip_last_error().decode()}")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().slimt_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


# ---- op level (slimt::qmm / TensorOps) ---------------------------------------

def affine(x, W_nk, bias, a_quant: float, b_quant: float):
    """qmm::affine; bias=None gives qmm::dot. W_nk: int8 [N][K]."""
    x = _f32(x)
    W = np.ascontiguousarray(W_nk, dtype=np.int8)
    N, K = W.shape
    M = x.size // K
    b = None if bias is None else _f32(bias).reshape(-1)
    y = np.empty(x.shape[:-1] + (N,), dtype=np.float32)
    _chk(lib().slimt_hip_affine(_p(x), M, K, _p(W), N, _p(b), a_quant, b_quant, _p(y)))
    return y


def dot(x, W_nk, a_quant: float, b_quant: float):
    return affine(x, W_nk, None, a_quant, b_quant)


def affine_with_select(x, W_nk, bias, a_quant, b_quant, indices):
    x = _f32(x)
    W = np.ascontiguousarray(W_nk, dtype=np.int8)
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    N, K = W.shape
    M = x.size // K
    b = _f32(bias).reshape(-1)
    y = np.empty(x.shape[:-1] + (idx.size,), dtype=np.float32)
    _chk(lib().slimt_hip_affine_select(_p(x), M, K, _p(W), N, _p(b), a_quant, b_quant, _p(idx),
                                       idx.size, _p(y)))
    return y


def affine_acc_i32(x, W_nk, a_quant: float):
    x = _f32(x)
    W = np.ascontiguousarray(W_nk, dtype=np.int8)
    N, K = W.shape
    M = x.size // K
    acc = np.empty((M, N), dtype=np.int32)
    _chk(lib().slimt_hip_affine_acc_i32(_p(x), M, K, _p(W), N, a_quant, _p(acc)))
    return acc


def debug_tied_output_proof(wemb, multiplier: float) -> bool:
    """The load-time proof on an int8 table [V][D] alone (host code, no device): re-quantising the dequantised table
    by its multiplier gives every byte back."""
    w = np.ascontiguousarray(wemb, dtype=np.int8)
    rows, cols = w.shape
    out = C.c_int(0)
    _chk(lib().slimt_hip_debug_tied_output_proof(_p(w), rows, cols, float(multiplier), C.byref(out)))
    return bool(out.value)


def debug_fused_decode_lds_bytes(D: int, F: int, Ld: int, sentences_per_wg: int, kv24: bool = True, mid: int = 0, tight: bool = False,
                                 merged: bool = False, nt: bool = False, scores: bool = False, forced: bool = False,
                                 sampled: bool = False) -> dict:
    """The dynamic LDS the persistent decoder's launcher asks for (host code, no device): bytes, and whether the LayerNorm
    constants / the output layer's epilogue constants are resident in it."""
    n, ln, epi = C.c_size_t(0), C.c_int(0), C.c_int(0)
    flags = (1 if merged else 0) | (2 if nt else 0) | (4 if scores else 0) | (8 if forced else 0) | (16 if sampled else 0)
    _chk(lib().slimt_hip_debug_fused_decode_lds_bytes(D, F, Ld, sentences_per_wg, 1 if kv24 else 0, mid, 1 if tight else 0, flags,
                                                      C.byref(n), C.byref(ln), C.byref(epi)))
    return dict(bytes=int(n.value), ln_in_lds=bool(ln.value), epi_in_lds=bool(epi.value))


def prepare_weight_transposed(weights, quant_mult: float):
    w = _f32(weights)
    rows, cols = w.shape
    out = np.empty((rows, cols), dtype=np.int8)
    _chk(lib().slimt_hip_prepare_weight_transposed(_p(w), _p(out), quant_mult, cols, rows))
    return out


def prepare_weight_quantized_transposed(w_nk, rows: int, cols: int):
    w = np.ascontiguousarray(w_nk, dtype=np.int8)
    out = np.empty_like(w)
    _chk(lib().slimt_hip_prepare_weight_quantized_transposed(_p(w), _p(out), rows, cols))
    return out


def layer_norm(x, scale, bias, eps: float = 1e-6):
    x = _f32(x)
    s, b = _f32(scale).reshape(-1), _f32(bias).reshape(-1)
    cols = x.shape[-1]
    y = np.empty_like(x)
    _chk(lib().slimt_hip_layer_norm(_p(x), _p(s), _p(b), eps, x.size // cols, cols, _p(y)))
    return y


def softmax(x):
    x = _f32(x)
    cols = x.shape[-1]
    y = np.empty_like(x)
    _chk(lib().slimt_hip_softmax(_p(x), x.size // cols, cols, _p(y)))
    return y


def highway(x, y, g):
    x, y, g = _f32(x), _f32(y), _f32(g)
    out = np.empty_like(x)
    _chk(lib().slimt_hip_highway(_p(x), _p(y), _p(g), x.size, _p(out)))
    return out


def sdpa(q, k, v, mask, want_attn: bool = True):
    q, k, v, mask = _f32(q), _f32(k), _f32(v), _f32(mask)
    B, H, Tq, dh = q.shape
    S = k.shape[2]
    out = np.empty_like(q)
    attn = np.empty((B, H, Tq, S), dtype=np.float32) if want_attn else None
    _chk(lib().slimt_hip_sdpa(_p(q), _p(k), _p(v), _p(mask), B, H, Tq, S, dh, _p(out), _p(attn)))
    return out, attn


# ---- engine level --------------------------------------------------------------

class Model:
    """Device-resident slimt::Transformer (weights on one GPU)."""

    def __init__(self, model, device: int = 0):
        """model: slimt_amd.synth.Model (or anything with .params/.H/...)."""
        keep = []
        arr = (_Param * len(model.params))()
        for i, p in enumerate(model.params.values()):
            buf = np.frombuffer(p.payload(), dtype=np.uint8).copy()
            name = p.name.encode()
            keep += [buf, name]
            arr[i] = _Param(name, 0 if p.kind == "f32" else 1, p.rows, p.cols,
                            buf.ctypes.data_as(C.c_void_p), buf.nbytes)
        dims = _Dims(model.enc_layers, model.dec_layers, model.H)
        h = C.c_void_p()
        _chk(lib().slimt_hip_model_create(C.cast(arr, C.c_void_p), len(model.params),
                                          C.byref(dims), device, C.byref(h)))
        self.h = h
        self.device = device
        self.D, self.F, self.H, self.V = model.D, model.F, model.H, model.V
        self.Le, self.Ld = model.enc_layers, model.dec_layers

    @classmethod
    def from_bin(cls, blob: bytes, enc_layers: int, dec_layers: int, heads: int, device: int = 0) -> "Model":
        """slimt_hip_model_create_from_bin: the Marian .bin container as Transformer::Transformer receives it
        (Transformer.cc:87-94); the library locates the items itself."""
        self = cls.__new__(cls)
        buf = bytes(blob)
        dims = _Dims(enc_layers, dec_layers, heads)
        h = C.c_void_p()
        _chk(lib().slimt_hip_model_create_from_bin(buf, len(buf), C.byref(dims), device, C.byref(h)))
        self.h = h
        self.device = device
        d, f, v, hh = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _chk(lib().slimt_hip_model_info(h, C.byref(d), C.byref(f), C.byref(v), C.byref(hh)))
        self.D, self.F, self.V, self.H = d.value, f.value, v.value, hh.value
        self.Le, self.Ld = enc_layers, dec_layers
        return self

    def set_kv_cache_policy(self, policy: int):
        """0 = per launch (default), 1 = temporal, 2 = non-temporal K/V cache loads in the decoder."""
        _chk(lib().slimt_hip_model_set_kv_cache_policy(self.h, policy))

    def set_xcd_affinity(self, xcds: int):
        """0 = off (default); 1 / 2 / 4 = a batch's decoder tiles are claimed on that many home XCDs."""
        _chk(lib().slimt_hip_model_set_xcd_affinity(self.h, xcds))

    def set_kv_cache_format(self, fmt: int):
        """0 = packed K/V cache where supported, 20 bits per value where a sentence's accumulators fit and 24 elsewhere
        (default); 1 = always f32; 2 = packed, always 24 bits; 3 = f32 and the reference's literal dequantise-then-attend
        sequence (stage-wise decoder: for checking)."""
        _chk(lib().slimt_hip_model_set_kv_cache_format(self.h, fmt))

    def debug_kv_watch(self):
        """(switched to the 24-bit form for good, sentence-layers that needed it so far, sentence-layers cached so far)."""
        sw, w, t = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        _chk(lib().slimt_hip_debug_kv_watch(self.h, C.byref(sw), C.byref(w), C.byref(t)))
        return bool(sw.value), int(w.value), int(t.value)

    def debug_kv_narrow_limit(self, limit: int):
        """Accumulators must lie in [-limit, limit) for the 20-bit cache form (default and maximum 2**19)."""
        _chk(lib().slimt_hip_debug_kv_narrow_limit(self.h, int(limit)))

    def debug_kv_tight_limit(self, limit: int):
        """Signed accumulators must lie in [-limit, limit) for the 16-bit cache form (default and maximum 2**15; 0 = never tried)."""
        _chk(lib().slimt_hip_debug_kv_tight_limit(self.h, int(limit)))

    def debug_out_tied_exact(self) -> bool:
        """Whether the load proved the tied output layer byte-equal to the embedding table (the fused decoder then
        reads the next embedding row from the output layer's tile)."""
        out = C.c_int(0)
        _chk(lib().slimt_hip_debug_out_tied_exact(self.h, C.byref(out)))
        return bool(out.value)

    def set_kv_centres(self, centres):
        """The 16-bit cache form's per-column centres, int32 [Ld][2][D] (else calibrated from the first large batch)."""
        c = np.ascontiguousarray(centres, dtype=np.int32)
        _chk(lib().slimt_hip_model_set_kv_centres(self.h, c.ctypes.data_as(C.c_void_p), c.size))

    def debug_kv_centres(self, Ld: int, D: int):
        """The centres [Ld][2][D] once they exist, else None."""
        out, ready = np.zeros((Ld, 2, D), dtype=np.int32), C.c_int(0)
        _chk(lib().slimt_hip_debug_kv_centres(self.h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(ready)))
        return out if ready.value else None

    def debug_kv_tight_watch(self):
        """(mask of decoder layers that stopped trying the 16-bit form, missed[4], submitted[4])."""
        off, missed, sub = C.c_uint(0), (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
        _chk(lib().slimt_hip_debug_kv_tight_watch(self.h, C.byref(off), missed, sub))
        return int(off.value), [int(x) for x in missed], [int(x) for x in sub]

    def debug_kv_recalibrations(self, max_recalibrations: int = -1) -> int:
        """Generations of K/V centres started after the first (a layer's watch tripped and the engine re-calibrated instead
        of switching it off); max_recalibrations >= 0 sets how many it may start (default 2)."""
        g = C.c_int(0)
        _chk(lib().slimt_hip_debug_kv_recalibrations(self.h, C.byref(g), max_recalibrations))
        return int(g.value)

    def set_adaptive_decoder_rows(self, on: bool):
        """Decode mode 0: 8 or 4 sentences per decoder workgroup while CUs would idle (default on)."""
        _chk(lib().slimt_hip_model_set_adaptive_decoder_rows(self.h, 1 if on else 0))

    def set_decoder_budget(self, workgroups: int):
        """Admission of persistent decoders: ~`workgroups` decoder workgroups at a time (0 = no limit)."""
        _chk(lib().slimt_hip_model_set_decoder_budget(self.h, workgroups))

    def close(self):
        if getattr(self, "h", None):
            lib().slimt_hip_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Pinned:
    """A growing pinned host buffer (slimt_hip_host_alloc) seen as numpy arrays."""

    def __init__(self):
        self.ptr = C.c_void_p()
        self.nbytes = 0

    def array(self, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if n > self.nbytes:
            self.free()
            want = max(n, 2 * self.nbytes, 4096)
            _chk(lib().slimt_hip_host_alloc(want, C.byref(self.ptr)))
            self.nbytes = want
        raw = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(self.nbytes,))
        return raw[:n].view(dtype).reshape(shape)

    def free(self):
        if self.ptr:
            lib().slimt_hip_host_free(self.ptr)
            self.ptr = C.c_void_p()
            self.nbytes = 0


class Context:
    """One worker's stream + workspace (mirrors one slimt Async worker)."""

    def __init__(self, model: Model, max_batch: int, max_source_length: int, stream: int = 0,
                 max_tokens: int = 0):
        """max_tokens > 0: a token-budget workspace (slimt_hip_ctx_create_budget): any batch with
        B <= max_batch, S <= max_source_length and B * S <= max_tokens."""
        self.model = model
        h = C.c_void_p()
        if max_tokens:
            _chk(lib().slimt_hip_ctx_create_budget(model.h, max_batch, max_source_length, max_tokens,
                                                   C.c_void_p(stream) if stream else None, C.byref(h)))
        else:
            _chk(lib().slimt_hip_ctx_create(model.h, max_batch, max_source_length,
                                            C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.B = self.S = 0
        self.N = model.V
        self._pinned = {}  # name -> _Pinned (translate_pinned)

    def close(self):
        if getattr(self, "h", None):
            lib().slimt_hip_ctx_destroy(self.h)
            self.h = None
            for b in getattr(self, "_pinned", {}).values():
                b.free()
            self._pinned = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        _chk(lib().slimt_hip_ctx_stream(self.h, C.byref(s)))
        return s.value or 0

    def synchronize(self):
        _chk(lib().slimt_hip_ctx_synchronize(self.h))
        self._prefix_keep = []  # (the prefixes armed before are read by now)

    def set_decode_mode(self, mode: int):
        """0 = auto (persistent fused decoder when supported), 1 = step-wise launches."""
        _chk(lib().slimt_hip_ctx_set_decode_mode(self.h, mode))

    def set_encode_rows(self, rows: int):
        """Rows per workgroup of the persistent D = 256 encoder: 0 = auto, 32, 64."""
        _chk(lib().slimt_hip_ctx_set_encode_rows(self.h, rows))

    def set_scores(self, destinations):
        """slimt_hip_ctx_set_scores: arm per-token scores for the NEXT translate call -- one [B_j, Tmax_j] float32
        destination per batch, as addresses (ints; device pointers for the device calls) or numpy arrays (host calls).
        The translate wrappers below do this themselves when asked for scores."""
        addrs = [d.ctypes.data if isinstance(d, np.ndarray) else (int(d) if d else 0) for d in destinations]
        arr = (C.c_void_p * max(1, len(addrs)))(*[a or None for a in addrs])
        _chk(lib().slimt_hip_ctx_set_scores(self.h, arr, len(addrs)))

    def set_target_prefix(self, prefixes):
        """slimt_hip_ctx_set_target_prefix: arm forced target prefixes for the NEXT translate call -- one (ids [B_j, Tmax_j],
        lens [B_j]) pair per batch, as numpy uint32 arrays (host calls; kept alive here until the next arming) or
        addresses (ints: device pointers for the device calls). The translate wrappers below take `prefix=` and do this."""
        keep, ids, lens = [], [], []
        for p_ids, p_len in prefixes:
            for a, out in ((p_ids, ids), (p_len, lens)):
                if isinstance(a, np.ndarray):
                    if a.dtype != np.uint32 or not a.flags.c_contiguous:
                        raise ValueError("target prefix: C-contiguous uint32 arrays expected")
                    keep.append(a)
                    out.append(a.ctypes.data)
                else:
                    out.append(int(a) if a else 0)
        # host arrays stay referenced until synchronize(): an asynchronous call reads them (pinned) or copies them (pageable)
        # from its stream, and a temporary made above may have no other owner
        self._prefix_keep = getattr(self, "_prefix_keep", []) + keep
        n = len(ids)
        a_ids = (C.c_void_p * max(1, n))(*[a or None for a in ids])
        a_len = (C.c_void_p * max(1, n))(*[a or None for a in lens])
        _chk(lib().slimt_hip_ctx_set_target_prefix(self.h, a_ids, a_len, n))

    def set_sampling(self, temperature: float, keys=None):
        """slimt_hip_ctx_set_sampling: arm temperature sampling for the NEXT translate call. keys: one entry per batch --
        a numpy uint64 [B_j] array (host calls; kept alive here until synchronize()), an address (int: a device pointer for
        the device calls) or None (that batch's keys are its row indices); None alone: one batch with row-index keys.
        The translate wrappers below take `sampling=(temperature, keys)` and do this."""
        if keys is None:
            keys = [None]
        keep, addrs = [], []
        for k in keys:
            if isinstance(k, np.ndarray):
                if k.dtype != np.uint64 or not k.flags.c_contiguous or k.ndim != 1:
                    raise ValueError("sampling keys: a C-contiguous one-dimensional uint64 array expected")
                keep.append(k)
                addrs.append(k.ctypes.data)
            else:
                addrs.append(int(k) if k else 0)
        self._prefix_keep = getattr(self, "_prefix_keep", []) + keep  # (like the prefixes: read until synchronize())
        arr = (C.c_void_p * max(1, len(addrs)))(*[a or None for a in addrs])
        _chk(lib().slimt_hip_ctx_set_sampling(self.h, float(temperature), arr, len(addrs)))

    def set_sampling_truncation(self, top_k: int = 0, top_p: float = 1.0):
        """slimt_hip_ctx_set_sampling_truncation: truncate the NEXT translate call's sampling (armed with set_sampling) to
        the top_k largest columns (0: no top-k) and the nucleus of mass top_p (1.0: no top-p). The translate wrappers take
        `truncation=(top_k, top_p)` beside `sampling=` and do this."""
        _chk(lib().slimt_hip_ctx_set_sampling_truncation(self.h, int(top_k), float(top_p)))

    def set_fanout_consensus(self, max_order: int, beta2: int, best, utility):
        """slimt_hip_ctx_set_fanout_consensus: arm the consensus selection for the NEXT fan-out call -- best [B] uint32 and
        utility [N] float64, as numpy arrays (host calls; kept alive here until the next arming) or addresses (ints: device
        pointers for the device call). max_order = 0 with no arrays disarms. The translate_fanout* wrappers take
        `consensus=` and do this."""
        keep, addr = [], []
        for a, dt in ((best, np.uint32), (utility, np.float64)):
            if isinstance(a, np.ndarray):
                if a.dtype != dt or not a.flags.c_contiguous:
                    raise ValueError("consensus: C-contiguous uint32 best and float64 utility expected")
                keep.append(a)
                addr.append(a.ctypes.data)
            else:
                addr.append(int(a) if a else 0)
        self._consensus_keep = keep
        _chk(lib().slimt_hip_ctx_set_fanout_consensus(self.h, int(max_order), int(beta2), C.c_void_p(addr[0] or None),
                                                      C.c_void_p(addr[1] or None)))

    def _arm_consensus(self, consensus, B: int, N: int):
        """arms a host fan-out call's consensus=(max_order, beta2); returns its (best [B], utility [N]) arrays"""
        best, utility = np.full(B, NO_ROW, np.uint32), np.zeros(N, np.float64)
        self.set_fanout_consensus(int(consensus[0]), int(consensus[1]), best, utility)
        return best, utility

    @staticmethod
    def _sampling_host(sampling, B: int):
        """(temperature, keys uint64 [B] | None) of a host call's `sampling=` (shape checked)"""
        T, keys = sampling
        if keys is not None and not isinstance(keys, int):
            keys = np.ascontiguousarray(keys, dtype=np.uint64)
            if keys.shape != (B,):
                raise ValueError("sampling: keys of shape %s expected" % ((B,),))
        return float(T), keys

    @staticmethod
    def _prefix_host(prefix, B: int, T: int):
        """(ids [B, T], lens [B]) as C-contiguous uint32 arrays (shapes checked)"""
        p_ids = np.ascontiguousarray(prefix[0], dtype=np.uint32)
        p_len = np.ascontiguousarray(prefix[1], dtype=np.uint32)
        if p_ids.shape != (B, T) or p_len.shape != (B,):
            raise ValueError("prefix: ids of shape %s and lengths of shape %s expected" % ((B, T), (B,)))
        return p_ids, p_len

    @staticmethod
    def _scores_array(a, B: int, T: int):
        if a.dtype != np.float32 or a.shape != (B, T) or not a.flags.c_contiguous:
            raise ValueError("scores: a C-contiguous float32 array of shape %s expected" % ((B, T),))
        return a

    def plan(self, S: int):
        """(encoder_fused, decoder_fused) for source length S in the current mode."""
        e, d = C.c_int(0), C.c_int(0)
        _chk(lib().slimt_hip_ctx_plan(self.h, S, C.byref(e), C.byref(d)))
        return bool(e.value), bool(d.value)

    def translate(self, ids, lengths, shortlist=None, limit_factor: float = 1.5, eos_id: int = 0,
                  want_align: bool = False, scores: bool = False, prefix=None, sampling=None, truncation=None):
        """Model::forward. Returns out_ids [B,Tmax], out_len [B], align|None (+ scores [B,Tmax] float32 with
        scores=True: the log-probability of each recorded token, include/slimt_hip.h slimt_hip_ctx_set_scores).
        prefix: (ids [B,Tmax], lens [B]) uint32 -- forced target prefixes (slimt_hip_ctx_set_target_prefix).
        sampling: (temperature, keys uint64 [B] | None) -- temperature sampling under per-sentence keys
        (slimt_hip_ctx_set_sampling; None: the row indices); the other translate wrappers take it in the same form, the
        device ones with a device pointer for the keys, the _many_ ones with one entry per batch."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        B, S = ids.shape
        Tmax = int(np.float32(limit_factor) * np.float32(S))
        T = max(Tmax, 1)
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        out_ids = np.zeros((B, T), dtype=np.uint32)
        out_len = np.zeros(B, dtype=np.uint32)
        align = np.zeros((B, T, S), dtype=np.float32) if want_align else None
        sc = np.full((B, T), np.nan, dtype=np.float32) if scores else None
        pre = self._prefix_host(prefix, B, T) if prefix is not None else None
        if scores:
            self.set_scores([sc])
        if pre is not None:
            self.set_target_prefix([pre])
        if sampling is not None:
            sm_t, sm_keys = self._sampling_host(sampling, B)
            self.set_sampling(sm_t, [sm_keys])
        if truncation is not None:
            self.set_sampling_truncation(*truncation)
        _chk(lib().slimt_hip_translate(self.h, _p(ids), _p(lengths), B, S, _p(sl),
                                       0 if sl is None else sl.size, limit_factor, eos_id,
                                       _p(out_ids), _p(out_len), _p(align)))
        self._prefix_keep = []  # (a blocking call: done with its prefix)
        return (out_ids, out_len, align, sc) if scores else (out_ids, out_len, align)

    def pinned_buffers(self, B: int, S: int, limit_factor: float = 1.5, want_align: bool = False):
        """This context's pinned staging arrays for a [B,S] batch: (ids, lengths, out_ids, out_len, align|None)."""
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        pin = lambda name: self._pinned.setdefault(name, _Pinned())
        return (pin("ids").array(np.uint32, (B, S)), pin("len").array(np.uint32, (B,)),
                pin("out").array(np.uint32, (B, T)), pin("ol").array(np.uint32, (B,)),
                pin("al").array(np.float32, (B, T, S)) if want_align else None)

    def translate_async(self, bufs, shortlist=None, generator=None, limit_factor: float = 1.5, eos_id: int = 0,
                        scores=None, prefix=None, sampling=None, truncation=None):
        """slimt_hip_translate_async[_generated] on arrays from pinned_buffers() (already filled);
        synchronize() before reading the outputs. `generator`: a ShortlistGenerator -- the batch's
        lexical shortlist is then generated on this context's stream (Model.cc:117-120).
        scores: a float32 [B, Tmax] array (pinned: written in place) that receives the tokens' log-probabilities.
        prefix: (ids [B, Tmax], lens [B]) uint32 host arrays, kept alive until the next call arms another one."""
        p_ids, p_len, p_out, p_ol, p_al = bufs
        B, S = p_ids.shape
        if scores is not None:
            self._scores_array(scores, B, p_out.shape[1])
        pre = self._prefix_host(prefix, B, p_out.shape[1]) if prefix is not None else None
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        if scores is not None:  # (armed right before the call that takes it)
            self.set_scores([scores])
        if pre is not None:
            self.set_target_prefix([pre])
        if sampling is not None:
            sm_t, sm_keys = self._sampling_host(sampling, B)
            self.set_sampling(sm_t, [sm_keys])
        if truncation is not None:
            self.set_sampling_truncation(*truncation)
        if generator is not None:
            _chk(lib().slimt_hip_translate_async_generated(self.h, generator.h, _p(p_ids), _p(p_len), B, S,
                                                           limit_factor, eos_id, _p(p_out), _p(p_ol), _p(p_al)))
            return
        _chk(lib().slimt_hip_translate_async(self.h, _p(p_ids), _p(p_len), B, S, _p(sl), 0 if sl is None else sl.size,
                                             limit_factor, eos_id, _p(p_out), _p(p_ol), _p(p_al)))

    def translate_pinned(self, ids, lengths, shortlist=None, limit_factor: float = 1.5, eos_id: int = 0,
                         want_align: bool = False, generator=None, scores: bool = False, prefix=None, sampling=None, truncation=None):
        """translate() through this context's pinned staging buffers and slimt_hip_translate_async:
        the persistent kernels then read and write host memory themselves, no copy is queued (host
        pipelines with several contexts: copies of one stream wait behind other streams' kernels).
        Returns copies of out_ids [B,Tmax], out_len [B], align|None."""
        ids = np.asarray(ids)
        B, S = ids.shape
        bufs = self.pinned_buffers(B, S, limit_factor, want_align)
        bufs[0][...] = ids
        bufs[1][...] = lengths
        sc = self._pinned.setdefault("sc", _Pinned()).array(np.float32, bufs[2].shape) if scores else None
        self.translate_async(bufs, shortlist, generator, limit_factor, eos_id, scores=sc, prefix=prefix, sampling=sampling,
                             truncation=truncation)
        self.synchronize()
        out = bufs[2].copy(), bufs[3].copy(), (bufs[4].copy() if want_align else None)
        return out + (sc.copy(),) if scores else out

    def translate_generated(self, generator, ids, lengths, limit_factor: float = 1.5, eos_id: int = 0,
                            want_align: bool = False, scores: bool = False, prefix=None, sampling=None, truncation=None):
        """Model::forward with its shortlist step (slimt_hip_translate_generated): host arrays, blocking.
        prefix: as in translate()."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        B, S = ids.shape
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        out_ids = np.zeros((B, T), dtype=np.uint32)
        out_len = np.zeros(B, dtype=np.uint32)
        align = np.zeros((B, T, S), dtype=np.float32) if want_align else None
        sc = np.full((B, T), np.nan, dtype=np.float32) if scores else None
        pre = self._prefix_host(prefix, B, T) if prefix is not None else None
        if scores:
            self.set_scores([sc])
        if pre is not None:
            self.set_target_prefix([pre])
        if sampling is not None:
            sm_t, sm_keys = self._sampling_host(sampling, B)
            self.set_sampling(sm_t, [sm_keys])
        if truncation is not None:
            self.set_sampling_truncation(*truncation)
        _chk(lib().slimt_hip_translate_generated(self.h, generator.h, _p(ids), _p(lengths), B, S, limit_factor,
                                                 eos_id, _p(out_ids), _p(out_len), _p(align)))
        self._prefix_keep = []  # (a blocking call: done with its prefix)
        return (out_ids, out_len, align, sc) if scores else (out_ids, out_len, align)

    # ---- fan-out: N decoder rows over B sources encoded once (include/slimt_hip.h, slimt_hip_translate_fanout*) ----
    def _arm(self, N: int, scores, prefix, sampling, truncation, T: int):
        """arms a one-batch call's options, shaped by its N rows (right before the call that takes them)"""
        pre = self._prefix_host(prefix, N, T) if prefix is not None else None
        if scores is not None:
            self.set_scores([self._scores_array(scores, N, T)])
        if pre is not None:
            self.set_target_prefix([pre])
        if sampling is not None:
            sm_t, sm_keys = self._sampling_host(sampling, N)
            self.set_sampling(sm_t, [sm_keys])
        if truncation is not None:
            self.set_sampling_truncation(*truncation)

    def translate_fanout(self, ids, lengths, row_src, shortlist=None, limit_factor: float = 1.5, eos_id: int = 0,
                         want_align: bool = False, scores: bool = False, prefix=None, sampling=None, truncation=None,
                         consensus=None):
        """slimt_hip_translate_fanout: translate() with N decoder rows over the B sources ids [B,S] / lengths [B], encoded
        once; row_src [N] uint32 names each row's source. Returns out_ids [N,Tmax], out_len [N], align [N,Tmax,S] | None
        (+ scores [N,Tmax]). prefix, sampling, truncation: as in translate(), shaped by N. Every row is bit for bit its row
        of translate() on ids[row_src], lengths[row_src] in decode mode 1.
        consensus: (max_order, beta2) -- the call also selects each source's consensus row on the device
        (slimt_hip_ctx_set_fanout_consensus) and returns, last, best [B] uint32 and utility [N] float64."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        row_src = np.ascontiguousarray(row_src, dtype=np.uint32)
        if ids.ndim != 2 or lengths.shape != (ids.shape[0],) or row_src.ndim != 1:
            raise ValueError("translate_fanout: ids [B, S], lengths [B] and row_src [N] expected")
        (B, S), N = ids.shape, row_src.size
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        out_ids = np.zeros((N, T), dtype=np.uint32)
        out_len = np.zeros(N, dtype=np.uint32)
        align = np.zeros((N, T, S), dtype=np.float32) if want_align else None
        sc = np.full((N, T), np.nan, dtype=np.float32) if scores else None
        self._arm(N, sc, prefix, sampling, truncation, T)
        cs = self._arm_consensus(consensus, B, N) if consensus is not None else ()
        _chk(lib().slimt_hip_translate_fanout(self.h, _p(ids), _p(lengths), B, S, _p(row_src), N, _p(sl),
                                              0 if sl is None else sl.size, limit_factor, eos_id, _p(out_ids), _p(out_len),
                                              _p(align)))
        self._prefix_keep = []  # (a blocking call: done with its prefix)
        return ((out_ids, out_len, align, sc) if scores else (out_ids, out_len, align)) + tuple(cs)

    def fanout_buffers(self, B: int, S: int, N: int, limit_factor: float = 1.5, want_align: bool = False):
        """This context's pinned arrays for translate_fanout_async: (ids [B,S], lengths [B], row_src [N], out_ids [N,Tmax],
        out_len [N], align [N,Tmax,S] | None)."""
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        pin = lambda name: self._pinned.setdefault(name, _Pinned())
        return (pin("fo_ids").array(np.uint32, (B, S)), pin("fo_len").array(np.uint32, (B,)),
                pin("fo_src").array(np.uint32, (N,)), pin("fo_out").array(np.uint32, (N, T)),
                pin("fo_ol").array(np.uint32, (N,)), pin("fo_al").array(np.float32, (N, T, S)) if want_align else None)

    def translate_fanout_async(self, bufs, shortlist=None, generator=None, limit_factor: float = 1.5, eos_id: int = 0,
                               scores=None, prefix=None, sampling=None, truncation=None, consensus=None):
        """slimt_hip_translate_fanout_async[_generated] on (ids, lengths, row_src, out_ids, out_len, align | None) host arrays
        (already filled; those of fanout_buffers() are pinned); synchronize() before reading the outputs. scores: a float32
        [N, Tmax] array; prefix, sampling, truncation: as in translate_async(), shaped by N.
        consensus: (max_order, beta2) -- returns (best [B] uint32, utility [N] float64), filled like the other outputs."""
        ids, lengths, row_src, out_ids, out_len, align = bufs
        for a in (ids, lengths, row_src, out_ids, out_len):
            if a.dtype != np.uint32 or not a.flags.c_contiguous:
                raise ValueError("translate_fanout_async: C-contiguous uint32 arrays expected")
        (B, S), N = ids.shape, row_src.size
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        if lengths.shape != (B,) or out_ids.shape != (N, T) or out_len.shape != (N,):
            raise ValueError("translate_fanout_async: mismatched shapes")
        if align is not None and (align.dtype != np.float32 or align.shape != (N, T, S) or not align.flags.c_contiguous):
            raise ValueError("translate_fanout_async: a C-contiguous float32 align of shape %s expected" % ((N, T, S),))
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        self._arm(N, scores, prefix, sampling, truncation, T)
        cs = self._arm_consensus(consensus, B, N) if consensus is not None else None
        if generator is not None:
            _chk(lib().slimt_hip_translate_fanout_async_generated(self.h, generator.h, _p(ids), _p(lengths), B, S, _p(row_src),
                                                                  N, limit_factor, eos_id, _p(out_ids), _p(out_len), _p(align)))
            return cs
        _chk(lib().slimt_hip_translate_fanout_async(self.h, _p(ids), _p(lengths), B, S, _p(row_src), N, _p(sl),
                                                    0 if sl is None else sl.size, limit_factor, eos_id, _p(out_ids),
                                                    _p(out_len), _p(align)))
        return cs

    def translate_fanout_pinned(self, ids, lengths, row_src, shortlist=None, limit_factor: float = 1.5, eos_id: int = 0,
                                want_align: bool = False, generator=None, scores: bool = False, prefix=None, sampling=None,
                                truncation=None, consensus=None):
        """translate_fanout() through this context's pinned arrays and slimt_hip_translate_fanout_async; returns copies."""
        ids, row_src = np.asarray(ids), np.asarray(row_src)
        B, S = ids.shape
        bufs = self.fanout_buffers(B, S, row_src.size, limit_factor, want_align)
        bufs[0][...] = ids
        bufs[1][...] = lengths
        bufs[2][...] = row_src
        sc = self._pinned.setdefault("fo_sc", _Pinned()).array(np.float32, bufs[3].shape) if scores else None
        cs = self.translate_fanout_async(bufs, shortlist, generator, limit_factor, eos_id, scores=sc, prefix=prefix,
                                         sampling=sampling, truncation=truncation, consensus=consensus)
        self.synchronize()
        out = bufs[3].copy(), bufs[4].copy(), (bufs[5].copy() if want_align else None)
        return (out + (sc.copy(),) if scores else out) + tuple(cs or ())

    def translate_fanout_device(self, d_ids: int, d_lengths: int, B: int, S: int, d_row_src: int, N: int, d_shortlist: int,
                                n_shortlist: int, limit_factor: float, eos_id: int, d_out_ids: int, d_out_len: int,
                                d_align: int = 0, steps_hint: int = 0, scores: int = 0, prefix=None, sampling=None,
                                truncation=None, consensus=None):
        """slimt_hip_translate_fanout_device: device pointers (ints) in and out, like translate_device(); d_row_src [N]
        uint32 (a value >= B is taken as B - 1), outputs and options shaped by N. consensus: (max_order, beta2, d_best,
        d_utility) with the device pointers of best [B] uint32 and utility [N] float64."""
        vp = C.c_void_p
        if scores:  # (armed right before the call that takes it)
            self.set_scores([scores])
        if prefix is not None:
            self.set_target_prefix([prefix])
        if sampling is not None:  # (temperature, device pointer of the [N] uint64 keys or 0 / None)
            self.set_sampling(sampling[0], [sampling[1]])
        if truncation is not None:
            self.set_sampling_truncation(*truncation)
        if consensus is not None:
            self.set_fanout_consensus(*consensus)
        _chk(lib().slimt_hip_translate_fanout_device(self.h, vp(d_ids), vp(d_lengths), B, S, vp(d_row_src), N,
                                                     vp(d_shortlist) if n_shortlist else None, n_shortlist, limit_factor,
                                                     eos_id, vp(d_out_ids), vp(d_out_len), vp(d_align) if d_align else None,
                                                     steps_hint))

    # ---- beam search with n-best output (include/slimt_hip.h, slimt_hip_translate_beam*) ----
    @staticmethod
    def _beam_mode(mean, mode) -> int:
        return int(mode) if mode is not None else (1 if mean else 0)

    def translate_beam(self, ids, lengths, beam: int, shortlist=None, limit_factor: float = 1.5, eos_id: int = 0,
                       mean: bool = False, want_align: bool = False, want_scores: bool = True, mode=None):
        """slimt_hip_translate_beam: beam search over the B sources ids [B,S] / lengths [B] with `beam` slots each. Returns
        the n-best, best first: out_ids [B,beam,Tmax], out_len [B,beam] (0: a dead slot), totals [B,beam] (-inf: a dead
        slot), token_scores [B,beam,Tmax] | None, align [B,beam,Tmax,S] | None. mean: order by totals / out_len."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if ids.ndim != 2 or lengths.shape != (ids.shape[0],):
            raise ValueError("translate_beam: ids [B, S] and lengths [B] expected")
        B, S = ids.shape
        k = int(beam)
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        kk = max(k, 0)
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        out_ids = np.zeros((B, kk, T), dtype=np.uint32)
        out_len = np.zeros((B, kk), dtype=np.uint32)
        totals = np.zeros((B, kk), dtype=np.float32)
        sc = np.zeros((B, kk, T), dtype=np.float32) if want_scores else None
        align = np.zeros((B, kk, T, S), dtype=np.float32) if want_align else None
        _chk(lib().slimt_hip_translate_beam(self.h, _p(ids), _p(lengths), B, S, k, self._beam_mode(mean, mode), _p(sl),
                                            0 if sl is None else sl.size, limit_factor, eos_id, _p(out_ids), _p(out_len),
                                            _p(totals), _p(sc), _p(align)))
        return out_ids, out_len, totals, sc, align

    def beam_buffers(self, B: int, S: int, beam: int, limit_factor: float = 1.5, want_align: bool = False):
        """This context's pinned arrays for translate_beam_async: (ids [B,S], lengths [B], out_ids [B,beam,Tmax], out_len
        [B,beam], totals [B,beam], token_scores [B,beam,Tmax], align [B,beam,Tmax,S] | None)."""
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        pin = lambda name: self._pinned.setdefault(name, _Pinned())
        return (pin("bm_ids").array(np.uint32, (B, S)), pin("bm_len").array(np.uint32, (B,)),
                pin("bm_out").array(np.uint32, (B, beam, T)), pin("bm_ol").array(np.uint32, (B, beam)),
                pin("bm_tot").array(np.float32, (B, beam)), pin("bm_sc").array(np.float32, (B, beam, T)),
                pin("bm_al").array(np.float32, (B, beam, T, S)) if want_align else None)

    def translate_beam_async(self, bufs, shortlist=None, generator=None, limit_factor: float = 1.5, eos_id: int = 0,
                             mean: bool = False, mode=None):
        """slimt_hip_translate_beam_async[_generated] on (ids, lengths, out_ids, out_len, totals, token_scores | None,
        align | None) host arrays (already filled; those of beam_buffers() are pinned); synchronize() before reading."""
        ids, lengths, out_ids, out_len, totals, sc, align = bufs
        for a in (ids, lengths, out_ids, out_len):
            if a.dtype != np.uint32 or not a.flags.c_contiguous:
                raise ValueError("translate_beam_async: C-contiguous uint32 arrays expected")
        if ids.ndim != 2 or out_ids.ndim != 3:
            raise ValueError("translate_beam_async: ids [B, S] and out_ids [B, beam, Tmax] expected")
        (B, S), k = ids.shape, out_ids.shape[1]
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        if lengths.shape != (B,) or out_ids.shape != (B, k, T) or out_len.shape != (B, k):
            raise ValueError("translate_beam_async: mismatched shapes")
        for a, shape in ((totals, (B, k)), (sc, (B, k, T)), (align, (B, k, T, S))):
            if a is None and shape != (B, k):
                continue
            if a is None or a.dtype != np.float32 or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError("translate_beam_async: a C-contiguous float32 array of shape %s expected" % (shape,))
        m = self._beam_mode(mean, mode)
        if generator is not None:
            _chk(lib().slimt_hip_translate_beam_async_generated(self.h, generator.h, _p(ids), _p(lengths), B, S, k, m,
                                                                limit_factor, eos_id, _p(out_ids), _p(out_len), _p(totals),
                                                                _p(sc), _p(align)))
            return
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        _chk(lib().slimt_hip_translate_beam_async(self.h, _p(ids), _p(lengths), B, S, k, m, _p(sl), 0 if sl is None else sl.size,
                                                  limit_factor, eos_id, _p(out_ids), _p(out_len), _p(totals), _p(sc), _p(align)))

    def translate_beam_pinned(self, ids, lengths, beam: int, shortlist=None, limit_factor: float = 1.5, eos_id: int = 0,
                              mean: bool = False, want_align: bool = False, generator=None, mode=None):
        """translate_beam() through this context's pinned arrays and slimt_hip_translate_beam_async; returns copies."""
        ids = np.asarray(ids)
        B, S = ids.shape
        bufs = self.beam_buffers(B, S, int(beam), limit_factor, want_align)
        bufs[0][...] = ids
        bufs[1][...] = lengths
        for a in bufs[2:]:
            if a is not None:
                a[...] = 0
        self.translate_beam_async(bufs, shortlist, generator, limit_factor, eos_id, mean, mode)
        self.synchronize()
        return tuple(None if a is None else a.copy() for a in bufs[2:])

    def translate_beam_generated(self, generator, ids, lengths, beam: int, limit_factor: float = 1.5, eos_id: int = 0,
                                 mean: bool = False, want_align: bool = False, mode=None):
        """slimt_hip_translate_beam_async_generated on pageable arrays, waited for: the batch's lexical shortlist comes
        from `generator`. Returns what translate_beam() returns."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if ids.ndim != 2 or lengths.shape != (ids.shape[0],) or int(beam) < 0:
            raise ValueError("translate_beam_generated: ids [B, S], lengths [B] and a beam >= 0 expected")
        (B, S), k = ids.shape, int(beam)
        T = max(int(np.float32(limit_factor) * np.float32(S)), 1)
        bufs = (ids, lengths, np.zeros((B, k, T), np.uint32), np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32),
                np.zeros((B, k, T), np.float32), np.zeros((B, k, T, S), np.float32) if want_align else None)
        self.translate_beam_async(bufs, None, generator, limit_factor, eos_id, mean, mode)
        self.synchronize()
        return bufs[2:]

    def translate_beam_device(self, d_ids: int, d_lengths: int, B: int, S: int, beam: int, d_shortlist: int, n_shortlist: int,
                              limit_factor: float, eos_id: int, d_out_ids: int, d_out_len: int, d_totals: int,
                              d_token_scores: int = 0, d_align: int = 0, steps_hint: int = 0, mean: bool = False, mode=None):
        """slimt_hip_translate_beam_device: device pointers (ints) in and out, like translate_fanout_device()."""
        vp = C.c_void_p
        _chk(lib().slimt_hip_translate_beam_device(self.h, vp(d_ids), vp(d_lengths), B, S, int(beam), self._beam_mode(mean, mode),
                                                   vp(d_shortlist) if n_shortlist else None, n_shortlist, limit_factor, eos_id,
                                                   vp(d_out_ids), vp(d_out_len), vp(d_totals),
                                                   vp(d_token_scores) if d_token_scores else None,
                                                   vp(d_align) if d_align else None, steps_hint))

    @staticmethod
    def _score_host(ids, lengths, tgt_ids, tgt_len):
        """(ids [B,S], lengths [B], tgt_ids [B,T], tgt_len [B]) as C-contiguous uint32 arrays (shapes checked)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        tgt_ids = np.ascontiguousarray(tgt_ids, dtype=np.uint32)
        tgt_len = np.ascontiguousarray(tgt_len, dtype=np.uint32)
        if ids.ndim != 2 or tgt_ids.ndim != 2:
            raise ValueError("score: ids [B, S] and tgt_ids [B, T] expected")
        B = ids.shape[0]
        if lengths.shape != (B,) or tgt_ids.shape[0] != B or tgt_len.shape != (B,):
            raise ValueError("score: %d sentences, but lengths %s, tgt_ids %s, tgt_len %s"
                             % (B, lengths.shape, tgt_ids.shape, tgt_len.shape))
        return ids, lengths, tgt_ids, tgt_len

    def set_score_alternatives(self, k: int, alt_ids=None, alt_scores=None, rank=None):
        """slimt_hip_ctx_set_score_alternatives: arm the NEXT score call to report the k (<= MAX_ALTERNATIVES) best tokens of
        every target position and the target's rank. alt_ids [B,T,k] uint32, alt_scores [B,T,k] float32 | None, rank [B,T]
        uint32 | None: numpy arrays of the kind of that call's scores, or device pointers (ints) for score_device. k = 0
        disarms. The caller keeps the arrays alive until the call has finished."""
        ptr = lambda a: None if a is None else (C.c_void_p(a) if isinstance(a, int) else _p(a))
        _chk(lib().slimt_hip_ctx_set_score_alternatives(self.h, int(k), ptr(alt_ids), ptr(alt_scores), ptr(rank)))

    @staticmethod
    def _alternatives_arrays(arrays, B: int, T: int):
        """(alt_ids, alt_scores | None, rank | None) checked against [B, T, k] / [B, T]; returns k"""
        alt_ids, alt_scores, rank = arrays
        if alt_ids is None or alt_ids.dtype != np.uint32 or alt_ids.ndim != 3 or alt_ids.shape[:2] != (B, T) \
                or not alt_ids.flags.c_contiguous:
            raise ValueError("score alternatives: a C-contiguous uint32 alt_ids of shape (%d, %d, k) expected" % (B, T))
        k = alt_ids.shape[2]
        if not 1 <= k <= MAX_ALTERNATIVES:
            raise ValueError("score alternatives: k = %d is not in 1..%d" % (k, MAX_ALTERNATIVES))
        if alt_scores is not None and (alt_scores.dtype != np.float32 or alt_scores.shape != (B, T, k)
                                       or not alt_scores.flags.c_contiguous):
            raise ValueError("score alternatives: a C-contiguous float32 alt_scores of shape %s expected" % ((B, T, k),))
        if rank is not None and (rank.dtype != np.uint32 or rank.shape != (B, T) or not rank.flags.c_contiguous):
            raise ValueError("score alternatives: a C-contiguous uint32 rank of shape %s expected" % ((B, T),))
        return k

    @staticmethod
    def _alternatives_k(k):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_ALTERNATIVES:
            raise ValueError("score alternatives: k = %r is not an integer in 1..%d" % (k, MAX_ALTERNATIVES))
        return int(k)

    def score(self, ids, lengths, shortlist, tgt_ids, tgt_len, want_align: bool = False, fill=np.nan, alternatives=None):
        """slimt_hip_score: teacher-forced scoring of given targets in one pass over all target positions. tgt_ids [B,T],
        tgt_len [B] (<= T; T is the caller's, there is no limit_factor cap). Returns scores [B,T] float32 -- the natural-log
        softmax probability of tgt_ids[b,t] for t < tgt_len[b], -inf for a token outside the shortlist -- and align [B,T,S]
        (head 0 of the last decoder layer) or None. Entries the call does not write (t >= tgt_len[b], alignment columns
        j >= lengths[b]) keep `fill`. Blocking; nothing armed on the context for translate calls is used or consumed.
        alternatives = k (1..MAX_ALTERNATIVES): additionally returns alt_ids [B,T,k] uint32 (the k most probable ids,
        0xFFFFFFFF past the layer's valid columns), alt_scores [B,T,k] float32 (their log-probabilities) and rank [B,T] uint32
        (the target's place in that order, 0xFFFFFFFF outside the layer); unwritten entries hold 0xFFFFFFFF / `fill`."""
        ids, lengths, tgt_ids, tgt_len = self._score_host(ids, lengths, tgt_ids, tgt_len)
        (B, S), T = ids.shape, tgt_ids.shape[1]
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        sc = np.full((B, T), fill, dtype=np.float32)
        align = np.full((B, T, S), fill, dtype=np.float32) if want_align else None
        alt = None
        if alternatives:
            k = self._alternatives_k(alternatives)
            alt = (np.full((B, T, k), 0xFFFFFFFF, dtype=np.uint32), np.full((B, T, k), fill, dtype=np.float32),
                   np.full((B, T), 0xFFFFFFFF, dtype=np.uint32))
            self.set_score_alternatives(k, *alt)
        _chk(lib().slimt_hip_score(self.h, _p(ids), _p(lengths), B, S, _p(sl), 0 if sl is None else sl.size,
                                   _p(tgt_ids), _p(tgt_len), T, _p(sc), _p(align)))
        return (sc, align) + alt if alt else (sc, align)

    def score_buffers(self, B: int, S: int, T: int, want_align: bool = False):
        """This context's pinned arrays for score_async: (ids [B,S], lengths [B], tgt_ids [B,T], tgt_len [B],
        scores [B,T], align [B,T,S] | None)."""
        pin = lambda name: self._pinned.setdefault(name, _Pinned())
        return (pin("ids").array(np.uint32, (B, S)), pin("len").array(np.uint32, (B,)),
                pin("tg").array(np.uint32, (B, T)), pin("tl").array(np.uint32, (B,)),
                pin("sc").array(np.float32, (B, T)), pin("al").array(np.float32, (B, T, S)) if want_align else None)

    def score_alternatives_buffers(self, B: int, T: int, k: int):
        """This context's pinned arrays for score_async(..., alternatives=): (alt_ids [B,T,k], alt_scores [B,T,k], rank [B,T])."""
        pin = lambda name: self._pinned.setdefault(name, _Pinned())
        return (pin("ai").array(np.uint32, (B, T, k)), pin("as").array(np.float32, (B, T, k)),
                pin("ar").array(np.uint32, (B, T)))

    def score_async(self, bufs, shortlist=None, generator=None, alternatives=None):
        """slimt_hip_score_async[_generated] on (ids, lengths, tgt_ids, tgt_len, scores, align | None) host arrays (already
        filled; those of score_buffers() are pinned: read and, the scores, written in place); synchronize() before reading
        the outputs, and keep the arrays alive until then. generator: a ShortlistGenerator -- the batch's lexical shortlist.
        alternatives: k -- this context's pinned arrays of score_alternatives_buffers(), filled with 0xFFFFFFFF / NaN -- or
        the caller's (alt_ids, alt_scores | None, rank | None), of the kind of scores; the three arrays are returned."""
        ids, lengths, tgt_ids, tgt_len, sc, align = bufs
        for a, dt in ((ids, np.uint32), (lengths, np.uint32), (tgt_ids, np.uint32), (tgt_len, np.uint32), (sc, np.float32)):
            if a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("score_async: C-contiguous uint32 inputs and float32 scores expected")
        if ids.ndim != 2 or tgt_ids.ndim != 2:
            raise ValueError("score_async: ids [B, S] and tgt_ids [B, T] expected")
        (B, S), T = ids.shape, tgt_ids.shape[1]
        if lengths.shape != (B,) or tgt_ids.shape[0] != B or tgt_len.shape != (B,) or sc.shape != (B, T):
            raise ValueError("score_async: mismatched shapes")
        if align is not None and (align.dtype != np.float32 or align.shape != (B, T, S) or not align.flags.c_contiguous):
            raise ValueError("score_async: a C-contiguous float32 align of shape %s expected" % ((B, T, S),))
        alt = None
        if alternatives is not None and not (isinstance(alternatives, (int, np.integer)) and not alternatives):
            if isinstance(alternatives, (tuple, list)):
                alt = tuple(alternatives)
                if len(alt) != 3:
                    raise ValueError("score alternatives: (alt_ids, alt_scores | None, rank | None) expected")
                k = self._alternatives_arrays(alt, B, T)
            else:
                k = self._alternatives_k(alternatives)
                alt = self.score_alternatives_buffers(B, T, k)
                alt[0][...] = 0xFFFFFFFF
                alt[1][...] = np.nan
                alt[2][...] = 0xFFFFFFFF
            self.set_score_alternatives(k, *alt)
        if generator is not None:
            _chk(lib().slimt_hip_score_async_generated(self.h, generator.h, _p(ids), _p(lengths), B, S, _p(tgt_ids),
                                                       _p(tgt_len), T, _p(sc), _p(align)))
            return alt
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        _chk(lib().slimt_hip_score_async(self.h, _p(ids), _p(lengths), B, S, _p(sl), 0 if sl is None else sl.size,
                                         _p(tgt_ids), _p(tgt_len), T, _p(sc), _p(align)))
        return alt

    def score_device(self, d_ids: int, d_lengths: int, B: int, S: int, d_shortlist: int, n_shortlist: int,
                     d_tgt_ids: int, d_tgt_len: int, T: int, d_scores: int, d_align: int = 0, alternatives=None):
        """slimt_hip_score_device: device pointers (ints) in and out, asynchronous on this context's stream.
        alternatives: (k, d_alt_ids, d_alt_scores | 0, d_rank | 0), device pointers to [B,T,k] / [B,T]; returned as given."""
        vp = C.c_void_p
        if alternatives is not None:
            if len(alternatives) != 4:
                raise ValueError("score alternatives: (k, d_alt_ids, d_alt_scores | 0, d_rank | 0) expected")
            k, d_ai, d_as, d_ar = alternatives
            k = self._alternatives_k(k)
            if not d_ai:
                raise ValueError("score alternatives: d_alt_ids is 0")
            self.set_score_alternatives(k, int(d_ai), int(d_as) if d_as else None, int(d_ar) if d_ar else None)
        _chk(lib().slimt_hip_score_device(self.h, vp(d_ids), vp(d_lengths), B, S, vp(d_shortlist) if n_shortlist else None,
                                          n_shortlist, vp(d_tgt_ids), vp(d_tgt_len), T, vp(d_scores),
                                          vp(d_align) if d_align else None))
        return alternatives

    @staticmethod
    def _candidates_host(ids, lengths, tgt_ids, tgt_len, cand_src):
        """(ids [B,S], lengths [B], tgt_ids [N,T], tgt_len [N], cand_src [N]) as C-contiguous uint32 arrays (shapes checked)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        tgt_ids = np.ascontiguousarray(tgt_ids, dtype=np.uint32)
        tgt_len = np.ascontiguousarray(tgt_len, dtype=np.uint32)
        cand_src = np.ascontiguousarray(cand_src, dtype=np.uint32)
        if ids.ndim != 2 or tgt_ids.ndim != 2:
            raise ValueError("score_candidates: ids [B, S] and tgt_ids [N, T] expected")
        B, N = ids.shape[0], tgt_ids.shape[0]
        if lengths.shape != (B,) or tgt_len.shape != (N,) or cand_src.shape != (N,):
            raise ValueError("score_candidates: %d sources and %d candidates, but lengths %s, tgt_len %s, cand_src %s"
                             % (B, N, lengths.shape, tgt_len.shape, cand_src.shape))
        return ids, lengths, tgt_ids, tgt_len, cand_src

    def score_candidates(self, ids, lengths, shortlist, tgt_ids, tgt_len, cand_src, want_align: bool = False, fill=np.nan,
                         alternatives=None):
        """slimt_hip_score_candidates: score() for N candidate targets tgt_ids [N,T] / tgt_len [N] over B sources encoded once;
        cand_src [N] (< B, any order) names each candidate's source. Returns scores [N,T] and align [N,T,S] | None (+ the
        alternatives' alt_ids [N,T,k], alt_scores [N,T,k], rank [N,T]), bit for bit what score() returns on ids[cand_src]."""
        ids, lengths, tgt_ids, tgt_len, cand_src = self._candidates_host(ids, lengths, tgt_ids, tgt_len, cand_src)
        (B, S), (N, T) = ids.shape, tgt_ids.shape
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        sc = np.full((N, T), fill, dtype=np.float32)
        align = np.full((N, T, S), fill, dtype=np.float32) if want_align else None
        alt = None
        if alternatives:
            k = self._alternatives_k(alternatives)
            alt = (np.full((N, T, k), 0xFFFFFFFF, dtype=np.uint32), np.full((N, T, k), fill, dtype=np.float32),
                   np.full((N, T), 0xFFFFFFFF, dtype=np.uint32))
            self.set_score_alternatives(k, *alt)
        _chk(lib().slimt_hip_score_candidates(self.h, _p(ids), _p(lengths), B, S, _p(sl), 0 if sl is None else sl.size,
                                              _p(tgt_ids), _p(tgt_len), T, _p(cand_src), N, _p(sc), _p(align)))
        return (sc, align) + alt if alt else (sc, align)

    def score_candidates_buffers(self, B: int, S: int, N: int, T: int, want_align: bool = False):
        """This context's pinned arrays for score_candidates_async: (ids [B,S], lengths [B], tgt_ids [N,T], tgt_len [N],
        cand_src [N], scores [N,T], align [N,T,S] | None)."""
        pin = lambda name: self._pinned.setdefault(name, _Pinned())
        return (pin("ids").array(np.uint32, (B, S)), pin("len").array(np.uint32, (B,)),
                pin("tg").array(np.uint32, (N, T)), pin("tl").array(np.uint32, (N,)), pin("cs").array(np.uint32, (N,)),
                pin("sc").array(np.float32, (N, T)), pin("al").array(np.float32, (N, T, S)) if want_align else None)

    def score_candidates_async(self, bufs, shortlist=None, generator=None, alternatives=None):
        """slimt_hip_score_candidates_async[_generated] on (ids, lengths, tgt_ids, tgt_len, cand_src, scores, align | None) host
        arrays (already filled; those of score_candidates_buffers() are pinned: read and written in place); synchronize()
        before reading the outputs. alternatives: the caller's (alt_ids [N,T,k], alt_scores | None, rank | None), of the
        kind of scores; returned as given."""
        ids, lengths, tgt_ids, tgt_len, cand_src, sc, align = bufs
        for a, dt in ((ids, np.uint32), (lengths, np.uint32), (tgt_ids, np.uint32), (tgt_len, np.uint32),
                      (cand_src, np.uint32), (sc, np.float32)):
            if a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("score_candidates_async: C-contiguous uint32 inputs and float32 scores expected")
        if ids.ndim != 2 or tgt_ids.ndim != 2:
            raise ValueError("score_candidates_async: ids [B, S] and tgt_ids [N, T] expected")
        (B, S), (N, T) = ids.shape, tgt_ids.shape
        if lengths.shape != (B,) or tgt_len.shape != (N,) or cand_src.shape != (N,) or sc.shape != (N, T):
            raise ValueError("score_candidates_async: mismatched shapes")
        if align is not None and (align.dtype != np.float32 or align.shape != (N, T, S) or not align.flags.c_contiguous):
            raise ValueError("score_candidates_async: a C-contiguous float32 align of shape %s expected" % ((N, T, S),))
        alt = None
        if alternatives is not None:
            alt = tuple(alternatives)
            if len(alt) != 3:
                raise ValueError("score alternatives: (alt_ids, alt_scores | None, rank | None) expected")
            self.set_score_alternatives(self._alternatives_arrays(alt, N, T), *alt)
        if generator is not None:
            _chk(lib().slimt_hip_score_candidates_async_generated(self.h, generator.h, _p(ids), _p(lengths), B, S, _p(tgt_ids),
                                                                  _p(tgt_len), T, _p(cand_src), N, _p(sc), _p(align)))
            return alt
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        _chk(lib().slimt_hip_score_candidates_async(self.h, _p(ids), _p(lengths), B, S, _p(sl), 0 if sl is None else sl.size,
                                                    _p(tgt_ids), _p(tgt_len), T, _p(cand_src), N, _p(sc), _p(align)))
        return alt

    def score_candidates_device(self, d_ids: int, d_lengths: int, B: int, S: int, d_shortlist: int, n_shortlist: int,
                                d_tgt_ids: int, d_tgt_len: int, T: int, d_cand_src: int, N: int, d_scores: int,
                                d_align: int = 0, alternatives=None):
        """slimt_hip_score_candidates_device: device pointers (ints) in and out, asynchronous on this context's stream.
        alternatives: (k, d_alt_ids, d_alt_scores | 0, d_rank | 0), device pointers to [N,T,k] / [N,T]; returned as given."""
        vp = C.c_void_p
        if alternatives is not None:
            if len(alternatives) != 4:
                raise ValueError("score alternatives: (k, d_alt_ids, d_alt_scores | 0, d_rank | 0) expected")
            k, d_ai, d_as, d_ar = alternatives
            k = self._alternatives_k(k)
            if not d_ai:
                raise ValueError("score alternatives: d_alt_ids is 0")
            self.set_score_alternatives(k, int(d_ai), int(d_as) if d_as else None, int(d_ar) if d_ar else None)
        _chk(lib().slimt_hip_score_candidates_device(self.h, vp(d_ids), vp(d_lengths), B, S,
                                                     vp(d_shortlist) if n_shortlist else None, n_shortlist, vp(d_tgt_ids),
                                                     vp(d_tgt_len), T, vp(d_cand_src), N, vp(d_scores),
                                                     vp(d_align) if d_align else None))
        return alternatives

    def candidates_rank_device(self, d_scores: int, d_tgt_len: int, d_cand_src: int, N: int, T: int, B: int, d_totals: int,
                               d_best: int, mean: bool = False):
        """slimt_hip_candidates_rank_device: candidates_rank over device arrays on this context's stream (totals [N] float32,
        best [B] uint32), e.g. behind score_candidates_device."""
        vp = C.c_void_p
        _chk(lib().slimt_hip_candidates_rank_device(self.h, vp(d_scores), vp(d_tgt_len), vp(d_cand_src), N, T, B,
                                                    int(bool(mean)), vp(d_totals), vp(d_best)))

    def consensus_select_device(self, d_ids: int, d_len: int, d_row_src: int, N: int, T: int, B: int, max_order: int,
                                beta2: int, d_utility: int, d_best: int):
        """slimt_hip_consensus_select_device: consensus_select over device arrays on this context's stream (utility [N]
        float64, best [B] uint32), e.g. behind translate_fanout_device."""
        vp = C.c_void_p
        _chk(lib().slimt_hip_consensus_select_device(self.h, vp(d_ids), vp(d_len), vp(d_row_src), N, T, B, int(max_order),
                                                     int(beta2), vp(d_utility), vp(d_best)))

    def translate_device(self, d_ids: int, d_lengths: int, B: int, S: int, d_shortlist: int,
                         n_shortlist: int, limit_factor: float, eos_id: int, d_out_ids: int,
                         d_out_len: int, d_align: int = 0, steps_hint: int = 0, scores: int = 0, prefix=None, sampling=None, truncation=None):
        """Device pointers (ints) in and out; asynchronous when steps_hint > 0. scores: a device pointer to
        [B, Tmax] floats for the tokens' log-probabilities (0 = none). prefix: (d_ids, d_lens) device pointers of a
        forced target prefix ([B, Tmax] and [B] uint32)."""
        vp = C.c_void_p
        args = (self.h, vp(d_ids), vp(d_lengths), B, S, vp(d_shortlist) if n_shortlist else None,
                n_shortlist, limit_factor, eos_id, vp(d_out_ids), vp(d_out_len),
                vp(d_align) if d_align else None, steps_hint)
        if scores:  # (armed right before the call that takes it)
            self.set_scores([scores])
        if prefix is not None:
            self.set_target_prefix([prefix])
        if sampling is not None:  # (temperature, device pointer of the [B] uint64 keys or 0 / None)
            self.set_sampling(sampling[0], [sampling[1]])
        if truncation is not None:
            self.set_sampling_truncation(*truncation)
        _chk(lib().slimt_hip_translate_device(*args))

    def translate_many_device(self, batches, S: int, limit_factor: float, eos_id: int, steps_hint: int = 0, generator=None,
                              scores=None, prefix=None, sampling=None, truncation=None):
        """slimt_hip_translate_many_device: `batches` = [(d_ids, d_lengths, B, d_shortlist, n_shortlist, d_out_ids,
        d_out_len, d_align[, S_j])] of device pointers (ints; 0 = none) -- ONE encoder and ONE decoder launch for all of them;
        S_j: that batch's own padded length (<= S; default S). scores: one device pointer per batch ([B_j, Tmax_j] floats).
        prefix: one (d_ids, d_lens) pair of device pointers per batch (forced target prefixes)."""
        if scores is not None and len(scores) != len(batches):
            raise ValueError(f"scores: {len(scores)} destinations for {len(batches)} batches")
        arr = (_Batch * len(batches))()
        for j, b in enumerate(batches):
            d_ids, d_len, B, d_sl, n_sl, d_out, d_ol, d_al = b[:8]
            arr[j] = _Batch(d_ids, d_len, B, b[8] if len(b) > 8 else 0, d_sl if n_sl else None, n_sl, d_out, d_ol, d_al or None)
        if scores is not None:  # (armed right before the call that takes it)
            self.set_scores(list(scores))
        if prefix is not None:
            self.set_target_prefix(list(prefix))
        if sampling is not None:  # (temperature, one device pointer of keys per batch | None)
            self.set_sampling(sampling[0], list(sampling[1]) if sampling[1] is not None else [None] * len(batches))
        if truncation is not None:
            self.set_sampling_truncation(*truncation)
        if generator is not None:
            _chk(lib().slimt_hip_translate_many_device_generated(self.h, generator.h, arr, len(batches), S, limit_factor, eos_id, steps_hint))
            return
        _chk(lib().slimt_hip_translate_many_device(self.h, arr, len(batches), S, limit_factor, eos_id, steps_hint))

    def translate_many_async(self, bufs_list, shortlist=None, limit_factor: float = 1.5, eos_id: int = 0, generator=None,
                             scores=None, prefix=None, sampling=None, truncation=None):
        """slimt_hip_translate_many_async on a list of pinned buffer tuples (ids, lengths, out_ids, out_len, align|None),
        one shortlist (host array) or none for all; synchronize() before reading the outputs.
        scores: one float32 [B_j, Tmax_j] array per batch (pinned: the merged launch writes them in place).
        prefix: one (ids [B_j, Tmax_j], lens [B_j]) pair of uint32 host arrays per batch."""
        pre = None
        if prefix is not None:
            if len(prefix) != len(bufs_list):
                raise ValueError(f"prefix: {len(prefix)} prefixes for {len(bufs_list)} batches")
            pre = [self._prefix_host(p, b[2].shape[0], b[2].shape[1]) for p, b in zip(prefix, bufs_list)]
        if scores is not None:
            if len(scores) != len(bufs_list):
                raise ValueError(f"scores: {len(scores)} arrays for {len(bufs_list)} batches")
            for a, b in zip(scores, bufs_list):
                self._scores_array(a, b[2].shape[0], b[2].shape[1])
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        arr = (_Batch * len(bufs_list))()
        S = max(b[0].shape[1] for b in bufs_list)  # the launch's padded length; a batch may be padded to fewer tokens
        for j, (p_ids, p_len, p_out, p_ol, p_al) in enumerate(bufs_list):
            arr[j] = _Batch(p_ids.ctypes.data, p_len.ctypes.data, p_ids.shape[0], p_ids.shape[1], None if sl is None else sl.ctypes.data,
                            0 if sl is None else sl.size, p_out.ctypes.data, p_ol.ctypes.data,
                            None if p_al is None else p_al.ctypes.data)
        self._many_keep = (arr, sl)
        if scores is not None:  # (armed right before the call that takes it)
            self.set_scores(list(scores))
        if pre is not None:
            self.set_target_prefix(pre)
        if sampling is not None:  # (temperature, one uint64 [B_j] host array of keys per batch | None)
            ks = sampling[1] if sampling[1] is not None else [None] * len(bufs_list)
            if len(ks) != len(bufs_list):
                raise ValueError(f"sampling: {len(ks)} key arrays for {len(bufs_list)} batches")
            self.set_sampling(sampling[0], [self._sampling_host((sampling[0], k), b[2].shape[0])[1] for k, b in zip(ks, bufs_list)])
        if truncation is not None:
            self.set_sampling_truncation(*truncation)
        if generator is not None:  # every batch's own lexical shortlist, generated inside the encoder launch
            _chk(lib().slimt_hip_translate_many_async_generated(self.h, generator.h, arr, len(bufs_list), S, limit_factor, eos_id))
            return
        _chk(lib().slimt_hip_translate_many_async(self.h, arr, len(bufs_list), S, limit_factor, eos_id))

    def translate_device_generated(self, gen: "ShortlistGenerator", d_ids: int, d_lengths: int, B: int,
                                   S: int, limit_factor: float, eos_id: int, d_out_ids: int,
                                   d_out_len: int, d_align: int = 0, steps_hint: int = 0, scores: int = 0, prefix=None, sampling=None, truncation=None):
        """Shortlist generation + translate, all on this context's stream. scores, prefix: as in translate_device."""
        vp = C.c_void_p
        args = (self.h, gen.h, vp(d_ids), vp(d_lengths), B, S, limit_factor, eos_id, vp(d_out_ids),
                vp(d_out_len), vp(d_align) if d_align else None, steps_hint)
        if scores:  # (armed right before the call that takes it)
            self.set_scores([scores])
        if prefix is not None:
            self.set_target_prefix([prefix])
        if sampling is not None:  # (temperature, device pointer of the [B] uint64 keys or 0 / None)
            self.set_sampling(sampling[0], [sampling[1]])
        if truncation is not None:
            self.set_sampling_truncation(*truncation)
        _chk(lib().slimt_hip_translate_device_generated(*args))

    def encode(self, ids, lengths, want_embed=False, want_layers=False):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        B, S = ids.shape
        D, Le = self.model.D, self.model.Le
        emb = np.empty((B, S, D), dtype=np.float32) if want_embed else None
        layers = np.empty((Le, B, S, D), dtype=np.float32) if want_layers else None
        out = np.empty((B, S, D), dtype=np.float32)
        _chk(lib().slimt_hip_encode(self.h, _p(ids), _p(lengths), B, S, _p(emb), _p(layers), _p(out)))
        self.B, self.S = B, S
        return out, emb, layers

    def decode_begin(self, shortlist=None):
        sl = None if shortlist is None else np.ascontiguousarray(shortlist, dtype=np.uint32)
        _chk(lib().slimt_hip_decode_begin(self.h, _p(sl), 0 if sl is None else sl.size))
        self.N = self.model.V if sl is None else sl.size

    def decode_step(self, prev=None, want_attn=True, want_states=True):
        """Decoder::step. Returns logits [B,N], attn [B,H,1,S], states [Ld,B,D]."""
        B, S, m = self.B, self.S, self.model
        pv = None if prev is None else np.ascontiguousarray(prev, dtype=np.uint32)
        logits = np.empty((B, self.N), dtype=np.float32)
        attn = np.empty((B, m.H, 1, S), dtype=np.float32) if want_attn else None
        states = np.empty((m.Ld, B, m.D), dtype=np.float32) if want_states else None
        _chk(lib().slimt_hip_decode_step(self.h, _p(pv), _p(logits), _p(attn), _p(states)))
        return logits, attn, states

    def debug_decode_stamps(self, step: int):
        """Read the previous run's phase stamps (ticks of 10 ns) and arm `step`."""
        out = np.zeros(64, dtype=np.uint64)
        _chk(lib().slimt_hip_debug_decode_stamps(self.h, step, _p(out), 64))
        return out

    def debug_cross_attention(self, layer: int, yq, B: int, S: int, heads: int, literal: bool = False):
        """The decoder's cross-attention proper on projected queries yq [B, D] over the current batch's f32 K/V cache
        (decode_begin first): (joined heads [B, D], probabilities [B, H, S]); literal = the reference's own sequence."""
        yq = np.ascontiguousarray(yq, dtype=np.float32)
        out = np.empty_like(yq)
        attn = np.empty((B, heads, S), dtype=np.float32)
        _chk(lib().slimt_hip_debug_cross_attention(self.h, layer, 1 if literal else 0, _p(yq), _p(out), _p(attn)))
        return out, attn

    def debug_break_shortlist_handoff(self, broken: bool, poll_limit: int = 1 << 24):
        """The waiters of an in-launch shortlist look for a publication that never comes (tests: the timeout path)."""
        _chk(lib().slimt_hip_debug_break_shortlist_handoff(self.h, 1 if broken else 0, int(poll_limit)))

    def debug_set_counters(self, value: int):
        """slimt_hip_debug_ctx_set_counters: the ticket and claim counters, their host bases and the shortlist hand-over's
        epoch as they would be after `value` (uint32) tickets (tests: the wrap-around at 2^32)."""
        _chk(lib().slimt_hip_debug_ctx_set_counters(self.h, int(value) & 0xFFFFFFFF))

    def debug_shortlists(self, n_batches: int = 1, capacity: Optional[int] = None, with_counts: bool = False):
        """slimt_hip_debug_ctx_shortlists: the lists the last *_generated call left in this context, one uint32 array per
        sub-batch (one for an unmerged call) -- the first min(count, capacity) ids; capacity defaults to the vocabulary.
        with_counts: also the device's counts (uint32 [n_batches]), reported in full whatever the capacity."""
        cap = self.model.V if capacity is None else int(capacity)
        ids = np.zeros((max(n_batches, 1), max(cap, 1)), dtype=np.uint32)
        counts = np.zeros(max(n_batches, 1), dtype=np.uint32)
        _chk(lib().slimt_hip_debug_ctx_shortlists(self.h, n_batches, _p(ids), cap, _p(counts)))
        lists = [ids[j, : min(int(counts[j]), cap)].copy() for j in range(n_batches)]
        return (lists, counts) if with_counts else lists

    def debug_decoder_plan(self) -> dict:
        """The plan of this context's last fused decoder launch under the decoder admission (decoder_plan.h)."""
        out = np.zeros(6, dtype=np.int32)
        _chk(lib().slimt_hip_debug_decoder_plan(self.h, _p(out)))
        return dict(zip(("rows", "contexts", "in_flight", "n", "eighths", "queues"), (int(v) for v in out)))

    def debug_kv_formats(self, layers: int, max_batch: int):
        """[layers][B] uint8 of the last batch: 0 = its cache is in the 20-bit form, 1 = 24-bit; None when the batch's
        caches are all in one form."""
        out = np.zeros(layers * max_batch, dtype=np.uint8)
        b = C.c_size_t(0)
        _chk(lib().slimt_hip_debug_kv_formats(self.h, _p(out), out.size, C.byref(b)))
        if b.value == 0:
            return None
        return out[: layers * b.value].reshape(layers, b.value).copy()

    def profile_enable(self, kernel_id: int):
        _chk(lib().slimt_hip_profile_enable(self.h, kernel_id))

    def profile_reset(self):
        _chk(lib().slimt_hip_profile_reset(self.h))

    def profile_read(self):
        n = C.c_uint64(0)
        ms, macs, wbytes = C.c_double(0), C.c_double(0), C.c_double(0)
        _chk(lib().slimt_hip_profile_read(self.h, C.byref(n), C.byref(ms), C.byref(macs),
                                          C.byref(wbytes)))
        return {"launches": n.value, "total_ms": ms.value, "int8_macs": macs.value,
                "weight_bytes": wbytes.value}


class ShortlistGenerator:
    """slimt::ShortlistGenerator (Shortlist.hh:38-90) on the device."""

    def __init__(self, blob: bytes, source_vocab: int, target_vocab: int, shared: bool = False,
                 check: bool = False, device: int = 0):
        self.h = C.c_void_p()
        self.target_vocab = target_vocab
        buf = bytes(blob)
        _chk(lib().slimt_hip_shortlist_create(buf, len(buf), source_vocab, target_vocab, int(shared),
                                              int(check), device, C.byref(self.h)))
        f, b = C.c_uint64(), C.c_uint64()
        _chk(lib().slimt_hip_shortlist_info(self.h, C.byref(f), C.byref(b)))
        self.frequent, self.best = int(f.value), int(b.value)

    def generate(self, ids, lengths) -> np.ndarray:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        B, S = ids.shape
        out = np.zeros((self.target_vocab,), dtype=np.uint32)
        n = C.c_size_t()
        _chk(lib().slimt_hip_shortlist_generate(self.h, _p(ids), _p(lengths), B, S, _p(out), C.byref(n)))
        return out[: int(n.value)].copy()

    def generate_device(self, ctx: "Context", d_ids: int, d_lengths: int, B: int, S: int, d_out: int,
                        d_n: int) -> None:
        _chk(lib().slimt_hip_shortlist_generate_device(self.h, ctx.h, d_ids, d_lengths, B, S, d_out, d_n))

    def close(self):
        if self.h:
            lib().slimt_hip_shortlist_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass



# ---- the batching service (include/slimt_hip_service.h, libslimt_hip_host.so) -----------------------
_host_lib = None


def host_lib():
    """Load libslimt_hip_host.so (host/Service behind a C ABI; built by __graft_entry__.build())."""
    global _host_lib
    if _host_lib is not None:
        return _host_lib
    lib()  # libslimt_hip.so first: the host library links against it
    path = _build.HOST_LIB
    if not os.path.exists(path):
        raise SlimtHipError(f"{path} is missing: build it with `python -m slimt_amd.build`")
    H = C.CDLL(path)
    vp, sz = C.c_void_p, C.c_size_t
    H.slimt_hip_service_last_error.restype = C.c_char_p
    H.slimt_hip_service_create.argtypes = [vp, vp, sz, vp]
    H.slimt_hip_service_destroy.argtypes = [vp]
    H.slimt_hip_service_translate.argtypes = [vp, vp, vp, sz, vp]
    H.slimt_hip_result_view.argtypes = [vp] * 8
    H.slimt_hip_result_destroy.argtypes = [vp]
    H.slimt_hip_service_set_scores.argtypes = [vp, C.c_int]  # (include/slimt_hip_service_scores.h)
    H.slimt_hip_result_scores.argtypes = [vp, vp]
    H.slimt_hip_service_translate_prefixed.argtypes = [vp, vp, vp, vp, vp, sz, vp]  # (include/slimt_hip_service_prefix.h)
    H.slimt_hip_service_set_sampling.argtypes = [vp, C.c_float]  # (include/slimt_hip_service_sampling.h)
    H.slimt_hip_service_translate_sampled.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, sz, vp]
    H.slimt_hip_service_set_sampling_truncation.argtypes = [vp, C.c_uint32, C.c_float]
    H.slimt_hip_service_score.argtypes = [vp, vp, vp, vp, vp, sz, vp]  # (include/slimt_hip_service_score.h)
    H.slimt_hip_service_score_alternatives.argtypes = [vp, vp, vp, vp, vp, sz, C.c_uint32, vp]  # (include/slimt_hip_service_alternatives.h)
    H.slimt_hip_result_alternatives.argtypes = [vp, sz, vp, vp, vp, vp]
    H.slimt_hip_service_score_candidates.argtypes = [vp, vp, vp, sz, vp, vp, vp, C.c_int, vp]  # (include/slimt_hip_service_candidates.h)
    H.slimt_hip_result_candidates.argtypes = [vp, vp, vp]
    H.slimt_hip_service_translate_samples.argtypes = [vp, vp, vp, sz, sz, C.c_uint64, vp]  # (include/slimt_hip_service_samples.h)
    H.slimt_hip_result_samples.argtypes = [vp, vp]
    H.slimt_hip_service_translate_consensus.argtypes = [vp, vp, vp, sz, sz, C.c_uint64, C.c_int, C.c_int, vp]  # (include/slimt_hip_service_consensus.h)
    H.slimt_hip_result_consensus.argtypes = [vp, vp, vp]
    _host_lib = H
    return H


class _ServiceConfig(C.Structure):
    _fields_ = [("max_words", C.c_uint64), ("wrap_length", C.c_uint64), ("limit_factor", C.c_float),
                ("workers_per_device", C.c_uint32), ("pad_id", C.c_uint32), ("eos_id", C.c_uint32),
                ("alignments", C.c_int32), ("lexical_shortlist", C.c_void_p), ("lexical_shortlist_bytes", C.c_uint64),
                ("source_vocab", C.c_uint64), ("target_vocab", C.c_uint64), ("shortlist_shared_vocab", C.c_int32),
                ("shortlist_check", C.c_int32), ("shortlist", C.c_void_p), ("n_shortlist", C.c_uint64),
                ("merge_batches", C.c_uint64), ("merge_words", C.c_uint64)]


class ServiceResult:
    """One request's result (slimt_hip_result): flat arrays, views valid while this object lives.
    targets[target_offsets[i]:target_offsets[i+1]] = sentence i's target ids (EOS included);
    alignment(i) = its [target tokens, source tokens] matrix."""

    def __init__(self, handle, source_lengths):
        self.h = handle
        n = C.c_size_t()
        ptrs = [C.c_void_p() for _ in range(6)]
        rc = host_lib().slimt_hip_result_view(self.h, C.byref(n), *[C.byref(p) for p in ptrs])
        if rc:
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        self.n = n.value

        def arr(p, dtype, count):
            if not count or not p.value:
                return np.zeros(0, dtype)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count,))

        self.target_offsets = arr(ptrs[1], np.uint64, self.n + 1)
        self.targets = arr(ptrs[0], np.uint32, int(self.target_offsets[-1]) if self.n else 0)
        self.padded_length = arr(ptrs[2], np.uint32, self.n)
        self.batch = arr(ptrs[3], np.uint64, self.n)
        self.align_offsets = arr(ptrs[5], np.uint64, self.n + 1)
        self.alignments = arr(ptrs[4], np.float32, int(self.align_offsets[-1]) if self.n else 0)
        self.source_lengths = source_lengths
        # per target token (indexed like targets) when the service scores, else None (slimt_hip_result_scores)
        sp = C.c_void_p()
        if host_lib().slimt_hip_result_scores(self.h, C.byref(sp)):
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        self.scores = arr(sp, np.float32, int(self.target_offsets[-1]) if self.n else 0) if sp.value else None

    def target(self, i: int) -> np.ndarray:
        return self.targets[int(self.target_offsets[i]):int(self.target_offsets[i + 1])]

    def alternatives(self, i: int):
        """sentence i of a BatchService.score(..., alternatives=k) result (slimt_hip_result_alternatives): alt_ids [n_i, k]
        uint32, alt_scores [n_i, k] float32 and ranks [n_i] uint32 over its n_i target tokens; views valid while this object
        lives"""
        k, pi, ps, pr = C.c_uint32(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        if host_lib().slimt_hip_result_alternatives(self.h, i, C.byref(k), C.byref(pi), C.byref(ps), C.byref(pr)):
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        n = int(self.target_offsets[i + 1]) - int(self.target_offsets[i])

        def arr(p, dtype, shape):
            if not n or not p.value:
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=shape)

        return arr(pi, np.uint32, (n, k.value)), arr(ps, np.float32, (n, k.value)), arr(pr, np.uint32, (n,))

    def candidates(self, n_sources: int):
        """of a BatchService.score_candidates result (slimt_hip_result_candidates): (totals float32 [entries] -- each
        candidate's summed score --, best uint32 [n_sources] -- per source the index among its own candidates of the best
        one, 0xFFFFFFFF: none); views valid while this object lives"""
        pt, pb = C.c_void_p(), C.c_void_p()
        if host_lib().slimt_hip_result_candidates(self.h, C.byref(pt), C.byref(pb)):
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())

        def arr(p, dtype, count):
            if not count or not p.value:
                return np.zeros(0, dtype)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count,))

        return arr(pt, np.float32, self.n), arr(pb, np.uint32, int(n_sources))

    def consensus(self):
        """of a BatchService.translate_consensus result (slimt_hip_result_consensus): (utility float64 [entries] -- the
        winner's utility among its sentence's samples --, sample_index uint32 [entries] -- its index j among them); views
        valid while this object lives"""
        pu, pj = C.c_void_p(), C.c_void_p()
        if host_lib().slimt_hip_result_consensus(self.h, C.byref(pu), C.byref(pj)):
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())

        def arr(p, dtype):
            if not self.n or not p.value:
                return np.zeros(0, dtype)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(self.n,))

        return arr(pu, np.float64), arr(pj, np.uint32)

    def token_scores(self, i: int) -> np.ndarray:
        """sentence i's per-token log-probabilities (EOS included); the service must score"""
        if self.scores is None:
            raise SlimtHipError("the service does not score (BatchService(scores=True))")
        return self.scores[int(self.target_offsets[i]):int(self.target_offsets[i + 1])]

    def alignment(self, i: int) -> np.ndarray:
        a, b = int(self.align_offsets[i]), int(self.align_offsets[i + 1])
        rows = int(self.target_offsets[i + 1] - self.target_offsets[i])
        return self.alignments[a:b].reshape(rows, -1) if b > a else np.zeros((rows, 0), np.float32)

    def close(self):
        if getattr(self, "h", None):
            host_lib().slimt_hip_result_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchService:
    """host/Service over its C ABI: tokenised sentences in, target ids + alignment rows out; token-budget
    batches, double-buffered pinned workers, per-batch lexical shortlist on the device."""

    def __init__(self, models, max_words: int = 8192, wrap_length: int = 128, limit_factor: float = 1.5,
                 workers_per_device: int = 6, pad_id: int = 0, eos_id: int = 0, alignments: bool = True,
                 lexical_shortlist: bytes = b"", source_vocab: int = 0, target_vocab: int = 0,
                 shared_vocab: bool = False, check: bool = False, shortlist=None, merge_batches: int = 0, merge_words: int = 0,
                 scores: bool = False, temperature: float = 0.0, truncation=None):
        """temperature > 0: every request is sampled at that temperature (slimt_hip_service_set_sampling; translate(...,
        seed=)); truncation=(top_k, top_p): ... from the top_k largest columns and the nucleus of mass top_p
        (slimt_hip_service_set_sampling_truncation; such a service never merges batches). merge_batches / merge_words: merged launches (0 = the library's defaults: up to 8 consecutive batches of one padded
        length per launch pair within 8192 words; merge_batches = 1: never). scores: every result carries its target tokens'
        log-probabilities (ServiceResult.scores / token_scores; slimt_hip_service_set_scores)."""
        self._keep = []
        cfg = _ServiceConfig(max_words, wrap_length, limit_factor, workers_per_device, pad_id, eos_id,
                             1 if alignments else 0, None, 0, source_vocab, target_vocab,
                             1 if shared_vocab else 0, 1 if check else 0, None, 0, merge_batches, merge_words)
        if lexical_shortlist:
            buf = C.create_string_buffer(bytes(lexical_shortlist), len(lexical_shortlist))
            self._keep.append(buf)
            cfg.lexical_shortlist = C.cast(buf, C.c_void_p)
            cfg.lexical_shortlist_bytes = len(lexical_shortlist)
        elif shortlist is not None:
            sl = np.ascontiguousarray(shortlist, dtype=np.uint32)
            self._keep.append(sl)
            cfg.shortlist = sl.ctypes.data_as(C.c_void_p)
            cfg.n_shortlist = sl.size
        arr = (C.c_void_p * len(models))(*[m.h for m in models])
        self.h = C.c_void_p()
        if host_lib().slimt_hip_service_create(C.byref(cfg), arr, len(models), C.byref(self.h)):
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        if scores and host_lib().slimt_hip_service_set_scores(self.h, 1):
            err = host_lib().slimt_hip_service_last_error().decode()
            self.close()
            raise SlimtHipError(err)
        self.temperature = float(temperature)
        if temperature and host_lib().slimt_hip_service_set_sampling(self.h, float(temperature)):
            err = host_lib().slimt_hip_service_last_error().decode()
            self.close()
            raise SlimtHipError(err)
        if truncation is not None and host_lib().slimt_hip_service_set_sampling_truncation(
                self.h, int(truncation[0]), float(truncation[1])):
            err = host_lib().slimt_hip_service_last_error().decode()
            self.close()
            raise SlimtHipError(err)

    def translate_flat(self, tokens: np.ndarray, offsets: np.ndarray, prefix_tokens=None, prefix_offsets=None, seed=None) -> ServiceResult:
        """tokens uint32 (flat), offsets uint64 [n + 1]. Blocking; thread-safe. prefix_tokens / prefix_offsets: forced
        target prefixes in the same form (slimt_hip_service_translate_prefixed; an empty range: not forced). seed (a
        sampling service): sentence i is drawn under sampling_key(seed, i) (slimt_hip_service_translate_sampled)."""
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        out = C.c_void_p()
        if prefix_offsets is not None:
            prefix_tokens = np.ascontiguousarray(prefix_tokens, dtype=np.uint32)
            prefix_offsets = np.ascontiguousarray(prefix_offsets, dtype=np.uint64)
            if prefix_offsets.size != offsets.size:
                raise ValueError(f"prefixes: {prefix_offsets.size - 1} for {offsets.size - 1} sentences")
        if seed is not None:
            rc = host_lib().slimt_hip_service_translate_sampled(
                self.h, _p(tokens), _p(offsets), _p(prefix_tokens) if prefix_offsets is not None else None,
                _p(prefix_offsets) if prefix_offsets is not None else None, int(seed) & (2 ** 64 - 1), offsets.size - 1, C.byref(out))
        elif prefix_offsets is not None:
            rc = host_lib().slimt_hip_service_translate_prefixed(self.h, _p(tokens), _p(offsets), _p(prefix_tokens),
                                                                _p(prefix_offsets), offsets.size - 1, C.byref(out))
        else:
            rc = host_lib().slimt_hip_service_translate(self.h, _p(tokens), _p(offsets), offsets.size - 1, C.byref(out))
        if rc:
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        return ServiceResult(out, np.diff(offsets).astype(np.int64))

    @staticmethod
    def _flat(sentences):
        lens = np.fromiter((len(s) for s in sentences), dtype=np.uint64, count=len(sentences))
        offsets = np.zeros(len(sentences) + 1, np.uint64)
        np.cumsum(lens, out=offsets[1:])
        tokens = np.fromiter(itertools.chain.from_iterable(sentences), dtype=np.uint32, count=int(offsets[-1]))
        return tokens, offsets

    def translate(self, sentences, prefixes=None, seed=None) -> ServiceResult:
        """prefixes: one token list per sentence (empty: not forced) -- forced target prefixes; a given translation with
        its EOS is scored (include/slimt_hip_service_prefix.h). seed: on a sampling service (temperature=), the request's
        seed (include/slimt_hip_service_sampling.h; None: seed 0)."""
        if prefixes is None:
            return self.translate_flat(*self._flat(sentences), seed=seed)
        if len(prefixes) != len(sentences):
            raise ValueError(f"prefixes: {len(prefixes)} for {len(sentences)} sentences")
        return self.translate_flat(*self._flat(sentences), *self._flat(prefixes), seed=seed)

    def score(self, sentences, targets, alternatives: int = 0) -> ServiceResult:
        """slimt_hip_service_score: teacher-forced scoring of targets[i] (a token list, with its EOS when that is to be
        scored; any length) against sentences[i] in one pass over all target positions. The result's target(i) is the given
        tokens, token_scores(i) their log-probabilities (whether or not the service scores its translations),
        alignment(i) the [target tokens, source tokens] rows. Blocking; thread-safe.
        alternatives = k (1..MAX_ALTERNATIVES; slimt_hip_service_score_alternatives): the result's alternatives(i) are the
        k most probable ids of every target position, their log-probabilities and the given tokens' ranks."""
        if len(targets) != len(sentences):
            raise ValueError(f"targets: {len(targets)} for {len(sentences)} sentences")
        if alternatives:
            alternatives = Context._alternatives_k(alternatives)
        tokens, offsets = self._flat(sentences)
        t_tokens, t_offsets = self._flat(targets)
        out = C.c_void_p()
        if alternatives:
            rc = host_lib().slimt_hip_service_score_alternatives(self.h, _p(tokens), _p(offsets), _p(t_tokens), _p(t_offsets),
                                                                 offsets.size - 1, alternatives, C.byref(out))
        else:
            rc = host_lib().slimt_hip_service_score(self.h, _p(tokens), _p(offsets), _p(t_tokens), _p(t_offsets),
                                                    offsets.size - 1, C.byref(out))
        if rc:
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        return ServiceResult(out, np.diff(offsets).astype(np.int64))

    def score_candidates(self, sentences, candidates, mean: bool = False):
        """slimt_hip_service_score_candidates: candidates[i] is a list of token lists, the candidate translations of
        sentences[i] (any number, each with its EOS when that is to be scored); each sentence is encoded once. Returns
        (result, cand_offsets, totals, best): the ServiceResult has ONE ENTRY PER CANDIDATE in the order given -- sentence i's
        are entries cand_offsets[i] .. cand_offsets[i + 1] - 1, token_scores(e) / alignment(e) as score() gives them for the
        pair --, totals float32 [entries] their summed scores and best uint32 [len(sentences)] the index among a sentence's
        own candidates of the best one by the sum (mean=True: by the sum per token), 0xFFFFFFFF where none competes."""
        if len(candidates) != len(sentences):
            raise ValueError(f"candidates: {len(candidates)} lists for {len(sentences)} sentences")
        tokens, offsets = self._flat(sentences)
        t_tokens, t_offsets = self._flat([c for cs in candidates for c in cs])
        c_offsets = np.zeros(len(sentences) + 1, np.uint64)
        np.cumsum([len(cs) for cs in candidates], out=c_offsets[1:])
        out = C.c_void_p()
        if host_lib().slimt_hip_service_score_candidates(self.h, _p(tokens), _p(offsets), offsets.size - 1, _p(t_tokens),
                                                         _p(t_offsets), _p(c_offsets), int(bool(mean)), C.byref(out)):
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        res = ServiceResult(out, np.repeat(np.diff(offsets).astype(np.int64), np.diff(c_offsets).astype(np.int64)))
        totals, best = res.candidates(len(sentences))
        return res, c_offsets, totals, best

    def translate_samples(self, sentences, n: int, seed: int = 0) -> ServiceResult:
        """slimt_hip_service_translate_samples: n sampled translations of every sentence from one encoding of it, on a
        sampling service (temperature=; truncation= applies). The ServiceResult has ONE ENTRY PER SAMPLE -- sample j of
        sentence i is entry i * n + j, drawn under sampling_key(seed, i * n + j) --, token_scores(e) always filled.
        Blocking; thread-safe."""
        tokens, offsets = self._flat(sentences)
        out = C.c_void_p()
        if host_lib().slimt_hip_service_translate_samples(self.h, _p(tokens), _p(offsets), offsets.size - 1, int(n),
                                                          int(seed) & (2 ** 64 - 1), C.byref(out)):
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        res = ServiceResult(out, np.repeat(np.diff(offsets).astype(np.int64), int(n)))
        got = C.c_size_t(0)
        if host_lib().slimt_hip_result_samples(res.h, C.byref(got)) or got.value != int(n):
            raise SlimtHipError("translate_samples: the result holds %d samples per sentence, not %d" % (got.value, int(n)))
        return res

    def translate_consensus(self, sentences, n: int, seed: int = 0, max_order: int = 4, beta2: int = 4):
        """slimt_hip_service_translate_consensus: translate_samples(sentences, n, seed) followed by the consensus pick among
        each sentence's n samples, made on the device behind the fan-out call (no second encoding, no scorer pass). Returns
        (ServiceResult with ONE ENTRY PER SENTENCE -- the winning sample, token_scores(i) filled --, utility float64
        [sentences], sample_index uint32 [sentences]): entry i is entry i * n + sample_index[i] of translate_samples with the
        same seed. n <= 64. Blocking; thread-safe."""
        tokens, offsets = self._flat(sentences)
        out = C.c_void_p()
        if host_lib().slimt_hip_service_translate_consensus(self.h, _p(tokens), _p(offsets), offsets.size - 1, int(n),
                                                            int(seed) & (2 ** 64 - 1), int(max_order), int(beta2), C.byref(out)):
            raise SlimtHipError(host_lib().slimt_hip_service_last_error().decode())
        res = ServiceResult(out, np.diff(offsets).astype(np.int64))
        utility, index = res.consensus()
        return res, utility, index

    def close(self):
        if getattr(self, "h", None):
            host_lib().slimt_hip_service_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
