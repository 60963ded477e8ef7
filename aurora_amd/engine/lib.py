"""ctypes binding of libaurora_hip.so (include/aurora_hip.h).

PyTorch is used for device memory and streams only: every wrapper below takes torch CUDA
(HIP) tensors, checks what the C ABI cannot check (device, dtype, contiguity of the inner
dimension) and passes raw device pointers plus the current HIP stream.  A missing library is a
hard error -- there is no fallback implementation in this package.
"""

from __future__ import annotations

import ctypes
import os
import threading
from collections import namedtuple
from ctypes import c_float, c_int, c_int32, c_int64, c_void_p
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from aurora_amd.engine.tables import DeviceTables, _upload

F32, BF16, F64 = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2

_LIB_PATH = Path(__file__).resolve().parents[1] / "_lib" / "libaurora_hip.so"


class PatchVar(ctypes.Structure):
    _fields_ = [
        ("src", c_void_p), ("stride_b", c_int64), ("stride_t", c_int64), ("stride_c", c_int64),
        ("stride_h", c_int64), ("stride_w", c_int64), ("loc", c_void_p), ("inv_scale", c_void_p),
        ("transform", c_int32), ("tw0", c_float), ("tw1", c_float), ("tb", c_float),
    ]


class UnpatchVar(ctypes.Structure):
    _fields_ = [("dst", c_void_p), ("loc", c_void_p), ("scale", c_void_p),
                ("clamp_min0", c_int32), ("col0", c_int32), ("lvl_stride", c_int32), ("mod_col0", c_int32),
                ("prev", c_void_p), ("prev_sb", c_int64), ("prev_sc", c_int64), ("prev_sh", c_int64),
                ("inv_scale", c_void_p), ("clamp_max1_levels", ctypes.c_uint32),
                ("angle_col0", c_int32), ("dens_col0", c_int32), ("mask", c_void_p), ("mask_sh", c_int64),
                ("mask_thresh", c_float)]


def unpatch_var(dst: int, loc: int, scale: int, clamp_min0: int, col0: int) -> UnpatchVar:
    """An `aurora_unpatch_var` with every optional feature switched off."""
    d = UnpatchVar(dst, loc, scale, clamp_min0, col0)
    d.mod_col0 = d.angle_col0 = d.dens_col0 = -1
    return d


_SIGNATURES = {
    "aurora_hip_version": (c_int, []),
    "aurora_hip_last_error": (ctypes.c_char_p, []),
    "aurora_hip_default_f32_gemm": (c_int, []),
    "aurora_hip_linear_ex": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                     c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_int,
                                     c_int, c_int, c_void_p, c_float, c_void_p]),
    "aurora_hip_linear_workspace": (c_int64, [c_int64, c_int, c_int, c_int]),
    "aurora_hip_linear_ws": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                     c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p,
                                     c_int, c_int, c_void_p]),
    "aurora_hip_linear_batched": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int,
                                          c_int, c_int, c_int, c_int, c_void_p, c_float, c_int, c_int64, c_int64, c_int64,
                                          c_int64, c_void_p]),
    "aurora_hip_linear_plan": (c_int, [c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64,
                                       c_int64, c_int64, c_int64, c_int, c_int, c_int64, c_int, c_int,
                                       ctypes.POINTER(c_int32)]),
    "aurora_hip_absmax": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "aurora_hip_absmax_fold": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "aurora_hip_zero_words": (c_int, [c_void_p, c_int, c_void_p]),
    "aurora_hip_linear_layernorm": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_float,
                                            c_void_p]),
    "aurora_hip_split_f16": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_float, c_void_p]),
    "aurora_hip_layernorm_split": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int,
                                           c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_float, c_void_p]),
    "aurora_hip_linear": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                  c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_int,
                                  c_int, c_void_p]),
    "aurora_hip_window_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                            c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "aurora_hip_window_attention_planes": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                                   c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "aurora_hip_linear_planes": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int64,
                                         c_int, c_int, c_int, c_void_p]),
    "aurora_hip_gather_rows": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                       c_void_p]),
    "aurora_hip_layernorm": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                     c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_float,
                                     c_int, c_void_p]),
    "aurora_hip_merge_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                    c_int, c_float, c_int, c_void_p]),
    "aurora_hip_split_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "aurora_hip_patchify": (c_int, [ctypes.POINTER(PatchVar), c_int, c_void_p, c_int64, c_int, c_int,
                                    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "aurora_hip_patchify_absmax": (c_int, [ctypes.POINTER(PatchVar), c_int, c_void_p, c_int64, c_int, c_int,
                                           c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "aurora_hip_perceiver_attention": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64,
                                               c_int64, c_int64, c_int, c_int, c_int, c_int, c_int,
                                               c_void_p]),
    "aurora_hip_perceiver_attention_ex": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64,
                                                  c_int64, c_int64, c_int, c_int, c_int, c_int, c_int,
                                                  c_void_p, c_float, c_void_p]),
    "aurora_hip_perceiver_attention_unless": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64,
                                                      c_int64, c_int64, c_int, c_int, c_int, c_int, c_int,
                                                      c_void_p, c_float, c_void_p, c_float, c_void_p]),
    "aurora_hip_perceiver_out_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "aurora_hip_perceiver_probs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64,
                                           c_int, c_int, c_int, c_int, c_void_p, c_float, c_void_p]),
    "aurora_hip_perceiver_attention_scores": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int64, c_int64, c_int64,
                                                      c_int, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_float,
                                                      c_void_p]),
    "aurora_hip_perceiver_probs_scores": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_int64, c_int64,
                                                  c_int64, c_int, c_int, c_int, c_int, c_void_p, c_float, c_void_p]),
    "aurora_hip_perceiver_out": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                         c_int, c_int, c_int, c_int, c_int, c_void_p, c_float, c_void_p]),
    "aurora_hip_assemble_tokens": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int, c_int, c_int64, c_int, c_int, c_void_p]),
    "aurora_hip_unpatchify": (c_int, [c_void_p, c_int64, ctypes.POINTER(UnpatchVar), c_int, c_int,
                                      c_int, c_int, c_int, c_int, c_void_p]),
    "aurora_hip_copy2d": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int,
                                  c_void_p]),
    "aurora_hip_convert": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "aurora_hip_regrid_plan": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "aurora_hip_regrid": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                  c_void_p, c_int, c_void_p]),
    "aurora_hip_conservative_regrid": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_double,
                                               c_void_p]),
    "aurora_hip_scores_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int]),
    "aurora_hip_scores": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "aurora_hip_ensemble_scores_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int]),
    "aurora_hip_ensemble_scores": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "aurora_hip_ensemble_quantiles": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                              c_void_p]),
    "aurora_hip_spectra_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "aurora_hip_spectra": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_sphere_spectra_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "aurora_hip_sphere_spectra": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_sphere_analysis_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int]),
    "aurora_hip_sphere_analysis": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_sphere_synthesis_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int]),
    "aurora_hip_sphere_synthesis": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                            ctypes.c_size_t, c_void_p]),
    "aurora_hip_event_scores_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "aurora_hip_event_scores": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_field_stats_update": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_int, c_int,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "aurora_hip_probability_scores": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                              c_void_p]),
    "aurora_hip_diagnostics": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_double, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_void_p, c_int, c_int, c_void_p]),
    "aurora_hip_conditional_scores_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int]),
    "aurora_hip_conditional_scores": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int,
                                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "aurora_hip_region_scores_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int]),
    "aurora_hip_region_scores": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "aurora_hip_objects_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int]),
    "aurora_hip_objects": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_field_quantiles_workspace_bytes": (ctypes.c_size_t, [c_int, c_int]),
    "aurora_hip_field_quantiles": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                           c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_object_matches_workspace_bytes": (ctypes.c_size_t, [c_int64, c_int]),
    "aurora_hip_object_matches": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p,
                                          c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_nearest_event_workspace_bytes": (ctypes.c_size_t, [c_int64, c_int, c_int]),
    "aurora_hip_nearest_event": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int, ctypes.c_double, c_void_p, c_void_p,
                                         c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_object_separations": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p,
                                              c_void_p, c_void_p]),
    "aurora_hip_smooth_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int]),
    "aurora_hip_smooth": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                  ctypes.c_double, c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_extrema_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int]),
    "aurora_hip_extrema": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "aurora_hip_closed_contours": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "aurora_hip_link_extrema": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                        c_int, c_int, c_int, ctypes.c_double, c_void_p, c_void_p, c_void_p]),
}

_lib: Optional[ctypes.CDLL] = None


def library_path() -> Path:
    return _LIB_PATH


def load() -> ctypes.CDLL:
    """Load the HIP library once; raise if it has not been built."""
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise RuntimeError(
                f"{_LIB_PATH} is missing: build it with `python -m aurora_amd.build` "
                "(hipcc, gfx950). aurora_amd has no fallback compute path."
            )
        # (kernel experiments: AURORA_HIP_LIB points at an alternative build of the same ABI)
        lib = ctypes.CDLL(os.environ.get("AURORA_HIP_LIB") or str(_LIB_PATH))
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


class HipError(RuntimeError):
    pass


def _check(code: int) -> None:
    if code != 0:
        msg = load().aurora_hip_last_error().decode(errors="replace")
        # -1 = AURORA_E_ARG: the Python shim re-raises argument violations as the assertion /
        # value errors the reference raises for bad shapes.
        raise (ValueError if code == -1 else HipError)(f"libaurora_hip: {msg} (code {code})")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported compute dtype {dt}: the HIP engine computes in fp32 or bf16")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda, "tensor must live on the HIP device"
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _rows(t: torch.Tensor) -> tuple[int, int]:
    """(leading dimension in elements, inner size) of a 2-D view with unit inner stride."""
    assert t.dim() == 2 and t.stride(1) == 1, f"need a row-major 2-D view, got {t.shape} / {t.stride()}"
    if t.shape[0] == 1:  # the stride of a size-1 dimension is arbitrary (often 0): irrelevant here
        return max(t.stride(0), t.shape[1]), t.shape[1]
    return t.stride(0), t.shape[1]


# ---- optional per-launch timing (bench.py / tools): HIP events on the launch stream -----------
_profile: Optional[list] = None
_profile_only: Optional[set] = None


def profile_start(only: Optional[set] = None) -> None:
    """Start recording (kernel, algorithmic work, start event, stop event) for every launch, or for the
    kernels named in `only` (an event pair around a launch keeps it from overlapping its neighbours, so timing
    every launch of a step costs a few percent of the step)."""
    global _profile, _profile_only
    _profile = []
    _profile_only = only


def profile_stop() -> dict:
    """Stop recording; returns {kernel: {"launches", "ms", "work"}} (synchronises the device)."""
    global _profile
    rec, _profile = _profile or [], None
    torch.cuda.synchronize()
    out: dict = {}
    for name, work, e0, e1 in rec:
        d = out.setdefault(name, {"launches": 0, "ms": 0.0, "work": 0.0})
        d["launches"] += 1
        d["ms"] += e0.elapsed_time(e1)
        d["work"] += work
    return out


class _Timed:
    """Brackets one launch with HIP events when profiling is on (torch.cuda.Event records on the
    current stream, which is the stream every kernel of this library is launched on)."""

    def __init__(self, name: str, work: float):
        self.name, self.work = name, work

    def __enter__(self):
        self.on = _profile is not None and (_profile_only is None or self.name in _profile_only)
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if self.on:
            self.e1.record()
            _profile.append((self.name, self.work, self.e0, self.e1))
        return False


# ---- wrappers ------------------------------------------------------------------------------
# How fp32 linears issued by THIS thread are multiplied: (mode, guard tensor, guard limit); mode -1 = process default.
# Passed per call to aurora_hip_linear_ex -- the library itself keeps no mutable state, so two engines on different
# threads / streams cannot disturb each other, and nothing hidden is baked into a captured graph.
_f32 = threading.local()


def _f32_state():
    return getattr(_f32, "state", (-1, None, 0.0))


def default_f32_gemm() -> int:
    """The process default (AURORA_F32_GEMM=native|bf16|f16): 0 native fp32 MFMA, 1 three bf16 terms, 2 two fp16 terms."""
    return load().aurora_hip_default_f32_gemm()


class f32_gemm:
    """`with f32_gemm(mode):` -- fp32 linears issued by this thread inside use `mode` (0 native fp32 MFMA, 1 exact
    3 x bf16 operand splitting, 2 2 x fp16 splitting)."""

    def __init__(self, mode: int, guard=None):
        self.state = (mode, None if guard is None else guard[0], 0.0 if guard is None else float(guard[1]))

    def __enter__(self):
        self.prev = _f32_state()
        _f32.state = self.state

    def __exit__(self, *exc):
        _f32.state = self.prev
        return False


def absmax(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max |x| of a contiguous fp32 tensor into a one-element device tensor (no host synchronisation)."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(1, dtype=torch.float32, device=x.device) if out is None else out
    with _Timed("absmax", 0.0):
        _check(load().aurora_hip_absmax(_ptr(x), x.numel(), _ptr(out), _stream()))
    return out


class bounded_activations(f32_gemm):
    """`with bounded_activations():` -- the fp32 linears issued inside may use the 2 x fp16 operand split (three
    MFMAs instead of six, the same 2^-24 operand accuracy).  Without arguments the caller vouches that their
    activation operand is bounded by construction -- a LayerNorm output or the GELU of a linear of one -- i.e. far
    inside fp16's range (|x| < 65504) whatever the model's inputs are.  With `guard=(amax, limit)` the decision is
    taken on the device, per launch: fp16 terms iff `amax[0] < limit` (`amax` from `absmax`, or a bound derived from
    it), three bf16 terms otherwise.  Honours an explicit native / bf16 choice made through AURORA_F32_GEMM or an
    enclosing `f32_gemm(0)`."""

    def __init__(self, guard=None):
        super().__init__(2, guard)

    def __enter__(self):
        self.prev = _f32_state()
        explicit = self.prev[0] >= 0 or os.environ.get("AURORA_F32_GEMM") is not None
        _f32.state = self.prev if explicit else self.state


F32_A_SPLIT, F32_W_SPLIT, F32_C_SPLIT = 4, 8, 16   # include/aurora_hip.h: operands / output in the fp16-pair layout


def two_term_free() -> bool:
    """True unless the user pinned an fp32 GEMM mode (AURORA_F32_GEMM or an enclosing `f32_gemm`) -- the condition under
    which `bounded_activations` switches to the two-term split, and so the one for handing it pre-split operands."""
    return _f32_state()[0] < 0 and os.environ.get("AURORA_F32_GEMM") is None


def presplit_ok(n: int, k: int) -> bool:
    """Shapes the pre-split form of the two-term kernel takes (include/aurora_hip.h)."""
    return n % 256 == 0 and k % 32 == 0 and k >= 96


def split_f16(x: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 rows -> the fp16-pair layout of the two-term GEMMs (same shape, dtype float32 as a container: per 32
    features 32 high halves, then 32 remainders).  Weights take scale = 64."""
    assert x.dtype == torch.float32 and x.dim() == 2
    ld, K = _rows(x)
    out = torch.empty_like(x, memory_format=torch.contiguous_format) if out is None else out
    ldo, _ = _rows(out)
    _check(load().aurora_hip_split_f16(_ptr(x), ld, _ptr(out), ldo, x.shape[0], K, scale, _stream()))
    return out


def linear(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *,
           out2: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           act: int = ACT_NONE, n: Optional[int] = None, k: Optional[int] = None, presplit: int = 0) -> torch.Tensor:
    """out[M, N] = act(a[M, K] @ w[N, K].T + bias) (+ residual); all 2-D row-major views.
    `presplit`: F32_* flags -- which of a / w / out are in the fp16-pair layout (two-term mode only)."""
    lda, ka = _rows(a)
    ldw, kw = _rows(w)
    K = k if k is not None else ka
    N = n if n is not None else w.shape[0]
    M = a.shape[0]
    assert kw >= K and ka >= K and a.dtype == w.dtype == out.dtype, (a.dtype, w.dtype, out.dtype)
    assert out.shape[0] == M and out.shape[1] >= N
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() >= N and bias.is_contiguous())
    ldc, _ = _rows(out)
    ldc2 = ldr = 0
    if out2 is not None:
        assert out2.dtype != out.dtype and out2.shape[0] == M
        ldc2, _ = _rows(out2)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.shape[0] == M
        ldr, _ = _rows(residual)
    name = "linear_bf16" if a.dtype == torch.bfloat16 else "linear_f32"
    with _Timed(name, 2.0 * M * N * K):  # algorithmic FLOPs
        mode, guard, limit = _f32_state()
        if presplit:
            mode = 2 | presplit
        _check(load().aurora_hip_linear_ex(_ptr(a), lda, _ptr(w), ldw, _ptr(bias), _ptr(out), ldc, _ptr(out2),
                                           ldc2, _ptr(residual), ldr, M, N, K, dtype_code(a.dtype), act,
                                           mode, _ptr(guard), limit, _stream()))
    return out


def linear_workspace(M: int, N: int, K: int, dtype: torch.dtype = torch.bfloat16) -> int:
    """Bytes of scratch `linear_ws` would like for this shape (0: the library would not split it along K)."""
    return int(load().aurora_hip_linear_workspace(M, N, K, dtype_code(dtype)))


def linear_ws(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, workspace: torch.Tensor,
              tickets: torch.Tensor, *, split: int = 0, out2: Optional[torch.Tensor] = None,
              residual: Optional[torch.Tensor] = None, act: int = ACT_NONE) -> torch.Tensor:
    """`linear` with lent scratch: few-tile / long-K bf16 problems are split along K inside one launch (aurora_hip_linear_ws).
    `workspace`: any contiguous tensor; `tickets`: int32, zero on entry, left zero.  split = 0 lets the library choose."""
    lda, K = _rows(a)
    ldw, _ = _rows(w)
    M, N = a.shape[0], w.shape[0]
    assert a.dtype == w.dtype == out.dtype and tickets.dtype == torch.int32 and workspace.is_contiguous()
    ldc, _ = _rows(out)
    ldc2 = ldr = 0
    if out2 is not None:
        ldc2, _ = _rows(out2)
    if residual is not None:
        ldr, _ = _rows(residual)
    with _Timed("linear_bf16" if a.dtype == torch.bfloat16 else "linear_f32", 2.0 * M * N * K):
        _check(load().aurora_hip_linear_ws(_ptr(a), lda, _ptr(w), ldw, _ptr(bias), _ptr(out), ldc, _ptr(out2), ldc2,
                                           _ptr(residual), ldr, M, N, K, dtype_code(a.dtype), act, _ptr(workspace),
                                           workspace.numel() * workspace.element_size(), _ptr(tickets), tickets.numel(), split,
                                           _stream()))
    return out


def linear_batched(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *,
                   act: int = ACT_NONE) -> torch.Tensor:
    """out[g] = act(a[g] @ w[g].T + bias[g]) for every problem g of a strided batch, in one launch (aurora_hip_linear_batched).
    a (G, M, K), w (G, N, K), out (G, M, N): 3-D views with unit inner stride, any row and batch strides the C entry takes;
    a batch of one (or an `expand`ed operand: batch stride 0) shares that operand.  bias (G, >= N) fp32 or None.  The fp32
    mode and guard are this thread's (`f32_gemm`), as for `linear`."""
    assert a.dim() == w.dim() == out.dim() == 3 and a.dtype == w.dtype == out.dtype, (a.dtype, w.dtype, out.dtype)
    G, M, N, K = out.shape[0], a.shape[1], w.shape[1], a.shape[2]
    assert w.shape[2] == K and out.shape[1] == M and out.shape[2] == N
    for t in (a, w):
        assert t.shape[0] in (1, G) and t.stride(2) == 1, (t.shape, t.stride())
    assert out.stride(2) == 1
    bstride = lambda t: 0 if t.shape[0] == 1 else t.stride(0)  # noqa: E731
    lda, _ = _rows(a[0])
    ldw, _ = _rows(w[0])
    ldc, _ = _rows(out[0])
    sb = 0
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.dim() == 2 and bias.shape[0] in (1, G) and bias.shape[1] >= N
        assert bias.stride(1) == 1
        sb = bstride(bias)
    name = "linear_bf16" if a.dtype == torch.bfloat16 else "linear_f32"
    with _Timed(name, 2.0 * G * M * N * K):
        mode, guard, limit = _f32_state()
        _check(load().aurora_hip_linear_batched(_ptr(a), lda, _ptr(w), ldw, _ptr(bias), _ptr(out), ldc, M, N, K,
                                                dtype_code(a.dtype), act, mode, _ptr(guard), limit, G, bstride(a),
                                                bstride(w), sb, bstride(out), _stream()))
    return out


PLAN_KERNELS = ("f32_three", "f32_two", "f32_pp", "f32_pp_w", "f32_pp_aw", "f32_pp_w_tall", "f32_pp_aw_tall", "tile128",
                "ring", "ring_mid", "pp", "pp_splitk", "a4")   # include/aurora_hip.h: AURORA_PLAN_*, in order
LinearPlan = namedtuple("LinearPlan", "kernel twin bm bn ksplit vec_store")


def linear_plan(M: int, N: int, K: int, dtype: torch.dtype, *, f32_gemm: int = -1, guard: bool = False, batch: int = 1,
                ldc: Optional[int] = None, c_offset: int = 0, ldc2: Optional[int] = None, c2_offset: int = 0,
                ldr: Optional[int] = None, residual_offset: int = 0, workspace_bytes: int = -1, n_tickets: int = 0,
                split: int = 0, plane_stride: int = 0, plane_heads: int = 0, cus: int = 0) -> LinearPlan:
    """What `linear` and its siblings would launch for such a call, without launching (aurora_hip_linear_plan): the kernel by
    name (PLAN_KERNELS), whether a guarded two-term launch brings its three-term twin, the tile, the K split and whether
    the 16-byte store paths are taken.  f32_gemm as aurora_hip_linear_ex (-1: the process default; F32_* flags OR-ed in);
    ldc2 / ldr None = no second output / no residual (ldr = 0: a broadcast row); the *_offset are the bytes by which a base
    address misses 16-byte alignment; workspace_bytes >= 0 describes a `linear_ws` call.  cus = 0 plans for the current
    device and needs one; any other count is host arithmetic only."""
    out = (c_int32 * 6)()
    _check(load().aurora_hip_linear_plan(M, N, K, dtype_code(dtype), f32_gemm, int(guard), batch, N if ldc is None else ldc,
                                         16 + c_offset, ldc2 or 0, 0 if ldc2 is None else 16 + c2_offset, ldr or 0,
                                         0 if ldr is None else 16 + residual_offset, workspace_bytes, n_tickets, split,
                                         plane_stride, plane_heads, cus, out))
    return LinearPlan(PLAN_KERNELS[out[0]], bool(out[1]), out[2], out[3], out[4], bool(out[5]))


def linear_layernorm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], gain: Optional[torch.Tensor],
                     shift: Optional[torch.Tensor], x: torch.Tensor, x_out: torch.Tensor,
                     x_bf16: Optional[torch.Tensor], eps: float = 1e-5) -> torch.Tensor:
    """x_out = x + LN(a @ w.T + bias) * gain + shift, x_bf16 = bf16(x_out), in one launch (bf16 a / w, N = 512)."""
    lda, K = _rows(a)
    ldw, _ = _rows(w)
    M, N = a.shape[0], w.shape[0]
    assert a.dtype == w.dtype == torch.bfloat16 and x.dtype == x_out.dtype == torch.float32
    ldx, _ = _rows(x)
    ldo, _ = _rows(x_out)
    ldb = 0
    if x_bf16 is not None:
        assert x_bf16.dtype == torch.bfloat16
        ldb, _ = _rows(x_bf16)
    with _Timed("linear_layernorm_bf16", 2.0 * M * N * K):
        _check(load().aurora_hip_linear_layernorm(_ptr(a), lda, _ptr(w), ldw, _ptr(bias), _ptr(gain), _ptr(shift), _ptr(x),
                                                  ldx, _ptr(x_out), ldo, _ptr(x_bf16), ldb, M, N, K, eps, _stream()))
    return x_out


def linear_planes(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, sel0: int = 0) -> torch.Tensor:
    """out[h, m, sel0 + sel, :] = (a @ w.T + bias)[m, (sel * heads + h) * 64 : +64]: `out` is (heads, rows >= M, 3, 64) bf16 --
    q | k | v of a token next to each other, one attention head per plane.  `sel0` = 1: w holds the k | v rows only."""
    M, K = a.shape
    N = w.shape[0]
    heads = out.shape[0]
    assert a.dtype == w.dtype == out.dtype == torch.bfloat16 and a.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K
    assert out.dim() == 4 and out.shape[2:] == (3, 64) and out.shape[1] >= M and N == (3 - sel0) * 64 * heads
    assert out.stride(3) == 1 and out.stride(2) == 64 and out.stride(1) == 192   # (a row range of longer planes is fine)
    c = out[0, 0, sel0]
    with _Timed("linear_bf16", 2.0 * M * N * K):
        _check(load().aurora_hip_linear_planes(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(bias), _ptr(c), out.stride(0), heads,
                                               M, N, K, dtype_code(a.dtype), _stream()))
    return out


def window_attention(qkv: torch.Tensor, qkv_bias: Optional[torch.Tensor], out: torch.Tensor,
                     tok: torch.Tensor, grp: Optional[torch.Tensor], B: int, L: int, D: int,
                     heads: int, L_out: Optional[int] = None, planes: bool = False) -> torch.Tensor:
    """`L` rows of qkv per batch element ([owned | halo] for a latitude band), `L_out` rows of out.  `planes`: qkv is
    (heads, B * L, 3, 64), what `linear_planes` writes."""
    L_out = L if L_out is None else L_out
    if planes:
        assert qkv.is_contiguous() and qkv.shape == (heads, B * L, 3, 64) and qkv.dtype == torch.bfloat16
        assert out.numel() == B * L_out * D and out.dtype == qkv.dtype and tok.dtype == torch.int32 and tok.dim() == 2
        n_windows, n_tok = tok.shape
        # (the stride of a dimension of size 1 is arbitrary: a contiguous single plane may report 64)
        plane_stride = qkv.stride(0) if heads > 1 else B * L * 192
        with _Timed("window_attention_bf16", 4.0 * B * n_windows * n_tok * D * 2):
            _check(load().aurora_hip_window_attention_planes(_ptr(qkv), plane_stride, _ptr(qkv_bias), _ptr(out), _ptr(tok), _ptr(grp),
                                                             B, L, L_out, D, heads, n_windows, n_tok, dtype_code(qkv.dtype),
                                                             _stream()))
        return out
    assert qkv.is_contiguous() and out.is_contiguous() and qkv.numel() == B * L * 3 * D
    assert out.numel() == B * L_out * D and out.dtype == qkv.dtype
    assert tok.dtype == torch.int32 and tok.is_contiguous() and tok.dim() == 2
    assert grp is None or (grp.dtype == torch.uint8 and grp.shape == tok.shape and grp.is_contiguous())
    assert qkv_bias is None or (qkv_bias.dtype == torch.float32 and qkv_bias.numel() == 3 * D)
    n_windows, n_tok = tok.shape
    name = "window_attention_bf16" if qkv.dtype == torch.bfloat16 else "window_attention_f32"
    # algorithmic bytes: q, k, v read + o written once over the padded windows
    with _Timed(name, 4.0 * B * n_windows * n_tok * D * qkv.element_size()):
        _check(load().aurora_hip_window_attention(_ptr(qkv), _ptr(qkv_bias), _ptr(out), _ptr(tok), _ptr(grp),
                                                  B, L, L_out, D, heads, n_windows, n_tok,
                                                  dtype_code(qkv.dtype), _stream()))
    return out


def layernorm(y: torch.Tensor, gain: Optional[torch.Tensor], shift: Optional[torch.Tensor], *,
              res: Optional[torch.Tensor] = None, res_mod: int = 0,
              out_f32: Optional[torch.Tensor] = None, out_t: Optional[torch.Tensor] = None,
              eps: float = 1e-5, d: Optional[int] = None, split_t: bool = False, split_res: bool = False) -> None:
    """`split_t` / `split_res` (fp32 rows only, aurora_hip_layernorm_split): `out_t` receives the fp16-pair layout /
    `res` is in it."""
    ldy, dy = _rows(y)
    D = d if d is not None else dy
    M = y.shape[0]
    for v in (gain, shift):
        assert v is None or (v.dtype == torch.float32 and v.numel() >= D and v.is_contiguous())
    ldr = ldo = ldt = 0
    if res is not None:
        assert res.dtype == torch.float32
        ldr, _ = _rows(res)
    if out_f32 is not None:
        assert out_f32.dtype == torch.float32 and out_f32.shape[0] == M
        ldo, _ = _rows(out_f32)
    if out_t is not None:
        assert out_t.dtype == y.dtype and out_t.shape[0] == M
        ldt, _ = _rows(out_t)
    nbytes = M * D * (y.element_size() + (4 if res is not None else 0) + (4 if out_f32 is not None else 0)
                      + (y.element_size() if out_t is not None else 0))
    if split_t or split_res:
        assert y.dtype == torch.float32 and (out_t is not None) == split_t and (res is not None or not split_res)
        with _Timed("layernorm", float(nbytes)):
            _check(load().aurora_hip_layernorm_split(_ptr(y), ldy, _ptr(gain), _ptr(shift), _ptr(res), ldr, res_mod,
                                                     1 if split_res else 0, _ptr(out_f32), ldo, _ptr(out_t), ldt, M, D,
                                                     eps, _stream()))
        return
    with _Timed("layernorm", float(nbytes)):
        _check(load().aurora_hip_layernorm(_ptr(y), ldy, _ptr(gain), _ptr(shift), _ptr(res), ldr, res_mod,
                                           _ptr(out_f32), ldo, _ptr(out_t), ldt, M, D, eps,
                                           dtype_code(y.dtype), _stream()))


def merge_ln(x: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, out: torch.Tensor,
             B: int, C: int, H: int, W: int, D: int, eps: float = 1e-5) -> torch.Tensor:
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == B * C * H * W * D
    assert out.is_contiguous() and out.numel() == B * C * ((H + 1) // 2) * ((W + 1) // 2) * 4 * D
    with _Timed("merge_ln", 0.0):
        _check(load().aurora_hip_merge_ln(_ptr(x), _ptr(ln_w), _ptr(ln_b), _ptr(out), B, C, H, W, D, eps,
                                          dtype_code(out.dtype), _stream()))
    return out


def split_ln(y: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, out: torch.Tensor,
             B: int, C: int, H: int, W: int, Dq: int, crop_h: int, crop_w: int,
             eps: float = 1e-5) -> torch.Tensor:
    assert y.is_contiguous() and y.numel() == B * C * H * W * 4 * Dq and y.dtype == out.dtype
    assert out.is_contiguous() and out.numel() == B * C * (2 * H - crop_h) * (2 * W - crop_w) * Dq
    with _Timed("split_ln", 0.0):
        _check(load().aurora_hip_split_ln(_ptr(y), _ptr(ln_w), _ptr(ln_b), _ptr(out), B, C, H, W, Dq,
                                          crop_h, crop_w, eps, dtype_code(y.dtype), _stream()))
    return out


def patchify(desc: list[PatchVar], out: torch.Tensor, k_offset: int, k_total: int, B: int, T: int,
             n_lvl: int, Hp: int, Wp: int, P: int, absmax: Optional[torch.Tensor] = None) -> None:
    """`absmax` (one fp32 word, NOT zeroed here): max |value written| is folded into it."""
    Kpad = out.shape[1]
    assert out.is_contiguous() and out.shape[0] == n_lvl * B * Hp * Wp
    assert absmax is None or (absmax.dtype == torch.float32 and absmax.numel() >= 1)
    arr = (PatchVar * len(desc))(*desc)
    with _Timed("patchify", 0.0):
        _check(load().aurora_hip_patchify_absmax(arr, len(desc), _ptr(out), Kpad, k_offset, k_total, B, T, n_lvl,
                                                 Hp, Wp, P, dtype_code(out.dtype), _ptr(absmax), _stream()))


def perceiver_attention(q: torch.Tensor, q_col_stride: int, kv: torch.Tensor, out: torch.Tensor,
                        B: int, cols_per_b: int, kv_bstride: int, kv_lstride: int, Lq: int, Lk: int,
                        heads: int, head_dim: int, pair_guard=None, skip_guard=None) -> torch.Tensor:
    """`pair_guard=(word, limit)`: fp32 results are written as fp16 pairs iff word[0] < limit (decided on the device).
    `skip_guard=(word, limit)`: the launch retires at once iff word[0] < limit."""
    assert q.is_contiguous() and kv.is_contiguous() and out.is_contiguous()
    assert q.dtype == kv.dtype == out.dtype
    word, limit = pair_guard if pair_guard is not None else (None, 0.0)
    sword, slimit = skip_guard if skip_guard is not None else (None, 0.0)
    with _Timed("perceiver_attention", 0.0):
        _check(load().aurora_hip_perceiver_attention_unless(_ptr(q), q_col_stride, _ptr(kv), _ptr(out), B,
                                                            cols_per_b, kv_bstride, kv_lstride, Lq, Lk, heads,
                                                            head_dim, dtype_code(q.dtype), _ptr(word), float(limit),
                                                            _ptr(sword), float(slimit), _stream()))
    return out


def perceiver_probs(q: torch.Tensor, kv: torch.Tensor, B: int, cols_per_b: int, kv_bstride: int, kv_lstride: int,
                    Lq: int, Lk: int, heads: int, head_dim: int, guard=None):
    """Softmax weights P (n_cols, heads, 64) and the value rows as fp16 pairs Vp (n_cols * Lk, inner) of the
    re-associated decoder attention (aurora_hip_perceiver_probs)."""
    assert q.is_contiguous() and kv.is_contiguous() and q.dtype == kv.dtype == torch.float32
    n_cols, inner = B * cols_per_b, heads * head_dim
    P = torch.zeros((n_cols, heads, 64), device=kv.device, dtype=torch.float32)
    Vp = torch.zeros((n_cols * Lk, inner), device=kv.device, dtype=torch.float32)
    word, limit = guard if guard is not None else (None, 0.0)
    with _Timed("perceiver_attention", 0.0):
        _check(load().aurora_hip_perceiver_probs(_ptr(q), _ptr(kv), _ptr(P), _ptr(Vp), B, cols_per_b, kv_bstride,
                                                 kv_lstride, Lq, Lk, heads, head_dim, _ptr(word), float(limit), _stream()))
    return P, Vp


def perceiver_attention_scores(vs: torch.Tensor, s_off: int, out: torch.Tensor, B: int, cols_per_b: int, kv_bstride: int,
                               kv_lstride: int, Lq: int, Lk: int, heads: int, head_dim: int, pair_guard=None,
                               skip_guard=None) -> torch.Tensor:
    """Perceiver attention from pre-multiplied scores: a row of `vs` is [v | ... | scores (Lq * heads) at s_off]
    (aurora_hip_perceiver_attention_scores)."""
    assert vs.is_contiguous() and out.is_contiguous() and vs.dtype == out.dtype == torch.float32
    word, limit = pair_guard if pair_guard is not None else (None, 0.0)
    sword, slimit = skip_guard if skip_guard is not None else (None, 0.0)
    with _Timed("perceiver_attention", 0.0):
        _check(load().aurora_hip_perceiver_attention_scores(_ptr(vs), vs.shape[1], s_off, _ptr(out), B, cols_per_b, kv_bstride,
                                                            kv_lstride, Lq, Lk, heads, head_dim, _ptr(word), float(limit),
                                                            _ptr(sword), float(slimit), _stream()))
    return out


def perceiver_probs_scores(vs: torch.Tensor, s_off: int, B: int, cols_per_b: int, kv_bstride: int, kv_lstride: int,
                           Lq: int, Lk: int, heads: int, head_dim: int, guard=None):
    """perceiver_probs from pre-multiplied scores (aurora_hip_perceiver_probs_scores)."""
    assert vs.is_contiguous() and vs.dtype == torch.float32
    n_cols, inner = B * cols_per_b, heads * head_dim
    P = torch.zeros((n_cols, heads, 64), device=vs.device, dtype=torch.float32)
    Vp = torch.zeros((n_cols * Lk, inner), device=vs.device, dtype=torch.float32)
    word, limit = guard if guard is not None else (None, 0.0)
    with _Timed("perceiver_attention", 0.0):
        _check(load().aurora_hip_perceiver_probs_scores(_ptr(vs), vs.shape[1], s_off, _ptr(P), _ptr(Vp), B, cols_per_b,
                                                        kv_bstride, kv_lstride, Lq, Lk, heads, head_dim, _ptr(word),
                                                        float(limit), _stream()))
    return P, Vp


def perceiver_out(Vp: torch.Tensor, w_pairs: torch.Tensor, P: torch.Tensor, out: torch.Tensor, n_cols: int, Lq: int,
                  Lk: int, heads: int, head_dim: int, bias: Optional[torch.Tensor] = None, guard=None) -> torch.Tensor:
    """out[col * Lq + l] = sum_h sum_j P[col, h, l, j] W[:, h] Vp[col * Lk + j, h] (aurora_hip_perceiver_out).
    `out` may be a column block of wider rows; `w_pairs` rows may be longer than heads * head_dim."""
    assert Vp.is_contiguous() and w_pairs.is_contiguous() and P.is_contiguous()
    ldo, N = _rows(out)
    word, limit = guard if guard is not None else (None, 0.0)
    with _Timed("perceiver_out", 2.0 * n_cols * Lk * N * heads * head_dim):
        _check(load().aurora_hip_perceiver_out(_ptr(Vp), _ptr(w_pairs), w_pairs.shape[1], _ptr(P), _ptr(bias), _ptr(out),
                                               ldo, n_cols, Lq, Lk, heads, head_dim, N, _ptr(word), float(limit),
                                               _stream()))
    return out


def assemble_tokens(surf: torch.Tensor, agg: torch.Tensor, pos_scale: torch.Tensor,
                    time_emb: torch.Tensor, out_f32: torch.Tensor, out_t: Optional[torch.Tensor],
                    B: int, Cl: int, L: int, D: int) -> None:
    for t in (surf, agg, pos_scale, time_emb, out_f32):
        assert t.dtype == torch.float32 and t.is_contiguous()
    code = BF16 if out_t is not None else F32
    with _Timed("assemble_tokens", 0.0):
        _check(load().aurora_hip_assemble_tokens(_ptr(surf), _ptr(agg), _ptr(pos_scale), _ptr(time_emb),
                                                 _ptr(out_f32), _ptr(out_t), B, Cl, L, D, code, _stream()))


def unpatchify(y: torch.Tensor, desc: list[UnpatchVar], B: int, n_lvl: int, Hp: int, Wp: int,
               P: int) -> None:
    ldy, _ = _rows(y)
    assert y.dtype == torch.float32
    arr = (UnpatchVar * len(desc))(*desc)
    with _Timed("unpatchify", 0.0):
        _check(load().aurora_hip_unpatchify(_ptr(y), ldy, arr, len(desc), B, n_lvl, Hp, Wp, P, _stream()))


def copy2d(src: torch.Tensor, dst: torch.Tensor, cols: Optional[int] = None) -> None:
    lds_, cs = _rows(src)
    ldd, _ = _rows(dst)
    assert src.dtype == dst.dtype and src.shape[0] == dst.shape[0]
    with _Timed("copy2d", 0.0):
        _check(load().aurora_hip_copy2d(_ptr(src), lds_, _ptr(dst), ldd, src.shape[0],
                                        cols if cols is not None else cs, dtype_code(src.dtype), _stream()))


def gather_rows(src: torch.Tensor, idx: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst[r] = src[idx[r]] for 2-D row-major views with equal row width (bytes multiple of 16)."""
    lds_, w = _rows(src)
    ldd, wd = _rows(dst)
    assert w == wd and src.dtype == dst.dtype and idx.dtype == torch.int32 and idx.is_contiguous()
    assert dst.shape[0] == idx.numel()
    es = src.element_size()
    with _Timed("gather_rows", 0.0):
        _check(load().aurora_hip_gather_rows(_ptr(src), lds_ * es, _ptr(idx), _ptr(dst), ldd * es, idx.numel(), w * es,
                                             _stream()))
    return dst


def convert(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    assert {src.dtype, dst.dtype} == {torch.float32, torch.bfloat16}
    with _Timed("convert", 0.0):
        _check(load().aurora_hip_convert(_ptr(src), _ptr(dst), src.numel(), dtype_code(src.dtype), _stream()))
    return dst


def regrid_plan(lat, lon, lat_new, lon_new) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Interpolation tables of `Batch.regrid` (aurora_hip_regrid_plan, host arithmetic): (rows (n_lat_new, 2) int32,
    row_w (n_lat_new,) float64, cols (n_lon_new, 2) int32, col_w (n_lon_new,) float64) for vector coordinates."""
    lat, lon, lat_new, lon_new = (np.ascontiguousarray(x, dtype=np.float64) for x in (lat, lon, lat_new, lon_new))
    assert lat.ndim == lon.ndim == lat_new.ndim == lon_new.ndim == 1, "regrid_plan: coordinates must be vectors"
    rows, cols = np.zeros((len(lat_new), 2), np.int32), np.zeros((len(lon_new), 2), np.int32)
    row_w, col_w = np.zeros(len(lat_new)), np.zeros(len(lon_new))
    _check(load().aurora_hip_regrid_plan(lat.ctypes.data, len(lat), lon.ctypes.data, len(lon), lat_new.ctypes.data,
                                         len(lat_new), lon_new.ctypes.data, len(lon_new), rows.ctypes.data,
                                         row_w.ctypes.data, cols.ctypes.data, col_w.ctypes.data))
    return rows, row_w, cols, col_w


def regrid(src: list[torch.Tensor], dst: list[torch.Tensor], rows: torch.Tensor, row_w: torch.Tensor,
           cols: torch.Tensor, col_w: torch.Tensor) -> None:
    """dst[i][..., r, c] = the bilinear regrid of src[i][..., :, :] for every plane of every pair, in ONE launch.

    src: contiguous (..., n_lat, n_lon) tensors, all fp32 or all fp64; dst: contiguous fp32 (..., n_rows, n_cols) with
    the same leading shape; the tables: device copies of `regrid_plan`'s (a slice rows[r0:r1], row_w[r0:r1] regrids
    output rows r0..r1-1 only)."""
    assert len(src) == len(dst) and src
    dt = src[0].dtype
    n_lat, n_lon = src[0].shape[-2:]
    n_rows, n_cols = rows.shape[0], cols.shape[0]
    assert dt in (torch.float32, torch.float64), f"regrid: sources must be fp32 or fp64, got {dt}"
    assert rows.dtype == cols.dtype == torch.int32 and row_w.dtype == col_w.dtype == torch.float64
    assert rows.shape == (n_rows, 2) and cols.shape == (n_cols, 2) and row_w.shape == (n_rows,) and col_w.shape == (n_cols,)
    assert all(t.is_contiguous() for t in (rows, row_w, cols, col_w))
    sp, dp = [], []
    for s_, d_ in zip(src, dst):
        assert s_.dtype == dt and s_.is_contiguous() and s_.shape[-2:] == (n_lat, n_lon), "regrid: bad source"
        assert d_.dtype == torch.float32 and d_.is_contiguous() and d_.shape == (*s_.shape[:-2], n_rows, n_cols), "regrid: bad output"
        assert s_.device == d_.device == rows.device, "regrid: every tensor must be on the same device"
        n = s_.numel() // (n_lat * n_lon) if s_.numel() else 0
        sp += [s_.data_ptr() + i * n_lat * n_lon * s_.element_size() for i in range(n)]
        dp += [d_.data_ptr() + i * n_rows * n_cols * 4 for i in range(n)]
    if not sp:
        return
    planes = torch.tensor([sp, dp], dtype=torch.int64).to(rows.device)
    with _Timed("regrid", 0.0):
        _check(load().aurora_hip_regrid(_ptr(planes[0]), F64 if dt == torch.float64 else F32, _ptr(planes[1]), len(sp),
                                        n_lat, n_lon, _ptr(rows), _ptr(row_w), n_rows, _ptr(cols), _ptr(col_w), n_cols,
                                        _stream()))


def conservative_regrid(src: list[torch.Tensor], out: torch.Tensor, tables, min_valid: float) -> None:
    """out[p] = the conservative regrid (aurora_amd/conservative.py has the rule) of plane p of `src`, the planes of its
    tensors counted one tensor after the other, in ONE aurora_hip_conservative_regrid launch.

    src: contiguous (..., n_lat, n_lon) tensors, all fp32 or all fp64; out: ONE contiguous fp32 (n_planes, n_rows, n_cols)
    tensor on their device; tables: the eight device tables of include/aurora_hip.h (row first / count / weights / measures,
    then the same of the columns).  The source plane-pointer table is cached by address as in `scores_sums`; the
    destination's is formed on the device from the address of `out`, which may therefore be a new tensor in every call,
    also during stream capture.  No workspace, and the host does not wait for the device."""
    row_first, row_count, row_w, row_m, col_first, col_count, col_w, col_m = tables
    assert src and out.dim() == 3 and out.dtype == torch.float32 and out.is_contiguous(), "conservative_regrid: bad output"
    dev, dt = out.device, src[0].dtype
    n_lat, n_lon = src[0].shape[-2:]
    n, n_rows, n_cols = out.shape
    assert dt in (torch.float32, torch.float64), f"conservative_regrid: sources must be fp32 or fp64, got {dt}"
    for t, d_, shape in ((row_first, torch.int32, (n_rows, 2)), (row_count, torch.int32, (n_rows,)), (row_w, torch.float64, None),
                         (row_m, torch.float64, (n_rows,)), (col_first, torch.int32, (n_cols, 2)),
                         (col_count, torch.int32, (n_cols,)), (col_w, torch.float64, None), (col_m, torch.float64, (n_cols,))):
        assert t.device == dev and t.dtype == d_ and t.is_contiguous() and (t.dim() == 1 if shape is None else tuple(t.shape) == shape), \
            "conservative_regrid: a table has the wrong device, dtype or shape"
    addresses = []
    for s_ in src:
        assert s_.device == dev and s_.dtype == dt and s_.is_contiguous() and tuple(s_.shape[-2:]) == (n_lat, n_lon), \
            "conservative_regrid: bad source"
        addresses += [s_.data_ptr() + i * n_lat * n_lon * s_.element_size() for i in range(s_.numel() // (n_lat * n_lon))]
    assert len(addresses) == n, f"conservative_regrid: the sources hold {len(addresses)} planes, out {n}"
    if n == 0:
        return
    planes = _planes("conservative_regrid", [], dev)
    planes.add("source", addresses)
    at = planes.upload()
    step = 4 * n_rows * n_cols
    dst = torch.arange(out.data_ptr(), out.data_ptr() + n * step, step, dtype=torch.int64, device=dev)
    moved = float(n) * (n_lat * n_lon * src[0].element_size() + step)
    _launch(dev, "conservative_regrid", moved, "aurora_hip_conservative_regrid", at["source"],
            F64 if dt == torch.float64 else F32, _ptr(dst), n, n_lat, n_lon, n_rows, n_cols, _ptr(row_first), _ptr(row_count),
            _ptr(row_w), _ptr(row_m), _ptr(col_first), _ptr(col_count), _ptr(col_w), _ptr(col_m), float(min_valid))


# ---- what the verification wrappers below share: the planes of a call, the operand checks, the launch ----------------------
def _upload_current(a: np.ndarray, device: torch.device) -> torch.Tensor:
    with torch.cuda.device(device):   # (a table is uploaded, as a kernel is launched, with its device current)
        return _upload(a, device)


_plane_tables = DeviceTables(256, _upload_current)   # plane addresses -> the plane-pointer arrays of a call
_twiddles = DeviceTables(64, _upload_current)        # n_lon -> the table of `spectra_twiddle`


def _plane_addresses(fn: str, fields: list[torch.Tensor], n_lat: int, n_lon: int, what: str) -> list[int]:
    """The address of every (n_lat, n_lon) plane of every tensor, in row-major order of the leading dimensions.  A plane
    must be row-major contiguous; the leading dimensions may have any strides (history slices and other views)."""
    out: list[int] = []
    for v in fields:
        assert v.dim() >= 2 and tuple(v.shape[-2:]) == (n_lat, n_lon), f"{fn}: a {what} field is {tuple(v.shape)}, not (..., {n_lat}, {n_lon})"
        assert v.dtype == torch.float32, f"{fn}: {what} fields must be fp32, got {v.dtype}"
        assert (n_lon == 1 or v.stride(-1) == 1) and (n_lat == 1 or v.stride(-2) == n_lon), \
            f"{fn}: the planes of a {what} field are not row-major contiguous (strides {v.stride()})"
        base, lead, strides = v.data_ptr(), v.shape[:-2], v.stride()[:-2]
        out += [base + 4 * sum(i * s for i, s in zip(idx, strides)) for idx in np.ndindex(*lead)]
    return out


class _Planes:
    """The plane-pointer arrays of one call, list after list in ONE device table, which is cached by the addresses (a roll-out
    passes the same tensors again and again, and a captured graph must find its table alive and unchanged at every replay):
    `n`, the planes of each checked list, and from `upload` the device address of the array of every list by its label --
    None for a list that was given as None."""

    def __init__(self, fn: str, dev: torch.device):
        self.fn, self.dev, self.n = fn, dev, 0
        self.addresses: list[int] = []
        self._offset: dict = {}   # label -> bytes from the start of the table, or None

    def add(self, what: str, addresses: Optional[list[int]]) -> None:
        """One more list, as ready addresses (0: the kernel gets NULL for that plane) or None.  The ONE place where the position
        of a list in the table is worked out: after the lists before it, eight bytes an address."""
        self._offset[what] = None if addresses is None else 8 * len(self.addresses)
        self.addresses += addresses or []

    def upload(self) -> dict:
        """{label: device address of that list's array, or None}; the table stays alive as long as this object."""
        self._table = _plane_tables.get((tuple(self.addresses),), self.dev, lambda: np.asarray(self.addresses, np.int64),
                                        f"{self.fn}: call once on these tensors before capturing a graph (the plane-pointer table "
                                        "is uploaded on the first call, which a captured graph cannot replay)")
        first = self._table.data_ptr()
        return {what: None if offset is None else first + offset for what, offset in self._offset.items()}


def _planes(fn: str, lists, dev: torch.device, anchor: str = "", n_lat: int = 0, n_lon: int = 0, like: int = 0) -> _Planes:
    """The `_Planes` of the labelled lists [(what, fields or None)] of a call, after what every plane binding checks of the lists
    that are given: the same length, every field on `dev` (the device of the argument `anchor`) and shaped like its counterpart
    in the given list `like`, every plane as `_plane_addresses` wants it.  A caller with lists of another kind `add`s them."""
    given = [fs for _, fs in lists if fs is not None]
    if given:
        first = given[like]
        assert all(len(fs) == len(first) for fs in given), f"{fn}: the lists differ in length"
        for fs in given:
            for v, p in zip(fs, first):
                assert v.device == dev, f"{fn}: every tensor must be on the device of {anchor}"
                assert v.shape == p.shape, f"{fn}: shapes differ ({tuple(v.shape)} against {tuple(p.shape)})"
    planes = _Planes(fn, dev)
    for what, fs in lists:
        planes.add(what, None if fs is None else _plane_addresses(fn, fs, n_lat, n_lon, what))
    if given:
        planes.n = len(planes.addresses) // len(given)
    return planes


def _operand(fn: str, name: str, t: torch.Tensor, dtype: torch.dtype, kind: str, *, dev: Optional[torch.device] = None,
             anchor: str = "", dim: Optional[int] = None, shape: Optional[tuple] = None) -> None:
    """`t` is a contiguous `dtype` tensor with `dim` dimensions or of `shape`, on `dev` (the device of the argument `anchor`) or,
    without one, on any device.  `kind` is what the message calls such a tensor."""
    assert (t.is_cuda if dev is None else t.device == dev) and t.dtype == dtype and t.is_contiguous() and \
        (dim is None or t.dim() == dim) and (shape is None or tuple(t.shape) == tuple(shape)), \
        f"{fn}: {name} must be a contiguous {kind} on the device" + (f" of {anchor}" if anchor else "")


def _label_maps(fn: str, name: str, labels: torch.Tensor) -> tuple:
    """`labels` is a stack of label maps on the device: (its device, (n_lat, n_lon), the leading shape)."""
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.dim() >= 2 and labels.is_contiguous(), \
        f"{fn}: {name} must be a contiguous (..., n_lat, n_lon) int32 tensor on the device"
    return labels.device, labels.shape[-2:], tuple(labels.shape[:-2])


_TENSOR = "{what} must be a contiguous {dtype} tensor of shape {shape} on the device of {anchor}"


def _like(fn: str, what: str, t: torch.Tensor, shape, dtype: torch.dtype, dev: torch.device, anchor: str, text: str = _TENSOR) -> None:
    """`t` is a contiguous `dtype` tensor of `shape` on `dev`, the device of the argument `anchor`."""
    assert t.device == dev and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous(), \
        f"{fn}: " + text.format(what=what, dtype=dtype, shape=tuple(shape), anchor=anchor)


def _outputs(fn: str, out, specs, dev: torch.device, anchor: str, text: str = _TENSOR) -> tuple:
    """The outputs of a call, `specs` = ((shape, dtype, name), ...): new tensors, or the caller's `out` after `_like`."""
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype, _ in specs)
    for t, (shape, dtype, what) in zip(out, specs):
        _like(fn, what, t, shape, dtype, dev, anchor, text)
    return out


def _workspace(fn: str, workspace: Optional[torch.Tensor], dev: torch.device, anchor: str, query, *sizes) -> torch.Tensor:
    """A new workspace of `query(*sizes)` bytes, or the caller's after a check of what the library cannot check."""
    if workspace is None:
        return torch.empty(query(*sizes), dtype=torch.uint8, device=dev)
    assert workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous(), \
        f"{fn}: the workspace must be a contiguous uint8 tensor on the device of {anchor}"
    return workspace


def _launch(dev: torch.device, name: str, work: float, entry: str, *args) -> None:
    """`entry(*args, the current stream of dev)` with `dev` current, timed as `name` when profiling is on."""
    with torch.cuda.device(dev):
        with _Timed(name, work):
            _check(getattr(load(), entry)(*args, _stream()))


# ---- verification sums (aurora_hip_scores) ----------------------------------------------------------------
def scores_workspace_bytes(n_planes: int, n_lat: int, n_lon: int) -> int:
    return int(load().aurora_hip_scores_workspace_bytes(n_planes, n_lat, n_lon))


def scores_sums(pred: list[torch.Tensor], truth: list[torch.Tensor], clim: Optional[list[torch.Tensor]],
                row_w: torch.Tensor) -> torch.Tensor:
    """The eight verification sums (include/aurora_hip.h: count, w, w d, w d^2, w |d|, w p' t', w p'^2, w t'^2) of every
    plane of `pred` against the same plane of `truth` (and of `clim`, or None), as an (n_planes, 8) fp64 tensor on the
    device, in ONE aurora_hip_scores call.

    pred / truth / clim: lists of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any
    leading strides, any 4-byte plane alignment), the same leading shapes in each list; row_w: (n_lat,) fp64 on that
    device.  Nothing of plane size is allocated and the host does not wait for the device."""
    _operand("scores_sums", "row_w", row_w, torch.float64, "fp64 vector", dim=1)
    dev, n_lat = row_w.device, row_w.shape[0]
    n_lon = pred[0].shape[-1] if pred else 1
    planes = _planes("scores_sums", [("prediction", pred), ("truth", truth), ("climatology", clim)], dev, "row_w", n_lat, n_lon)
    n = planes.n
    sums = torch.empty(n, 8, dtype=torch.float64, device=dev)
    if n == 0:
        return sums
    at = planes.upload()
    workspace = torch.empty(scores_workspace_bytes(n, n_lat, n_lon), dtype=torch.uint8, device=dev)
    _launch(dev, "scores", 0.0, "aurora_hip_scores", at["prediction"], at["truth"], at["climatology"], n, n_lat, n_lon,
            _ptr(row_w), _ptr(sums), _ptr(workspace))
    return sums


# ---- ensemble verification sums (aurora_hip_ensemble_scores) -------------------------------------------------------
ENSEMBLE_MAX_MEMBERS = 64


def ensemble_scores_workspace_bytes(n_members: int, n_planes: int, n_lat: int, n_lon: int) -> int:
    return int(load().aurora_hip_ensemble_scores_workspace_bytes(n_members, n_planes, n_lat, n_lon))


def ensemble_scores_sums(members: list[list[torch.Tensor]], truth: list[torch.Tensor],
                         row_w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The eight ensemble sums (include/aurora_hip.h: count, w, w e, w e^2, w |e|, w a, w g, w v) and the rank histogram of
    every plane of M members against the same plane of `truth`, in ONE aurora_hip_ensemble_scores call: an (n_planes, 8)
    fp64 tensor and an (n_planes, M + 2) int64 tensor (bins 0 .. M, then the ties) on the device.

    members: M lists (2 <= M <= 64), each like `truth`: fp32 (..., n_lat, n_lon) tensors on one device with row-major
    contiguous planes (any leading strides, any 4-byte plane alignment) and the leading shapes of `truth`; row_w: (n_lat,)
    fp64 on that device.  The plane-pointer table is cached by address as in `scores_sums`.  Nothing of plane size is
    allocated and the host does not wait for the device."""
    _operand("ensemble_scores_sums", "row_w", row_w, torch.float64, "fp64 vector", dim=1)
    M = len(members)
    assert 2 <= M <= ENSEMBLE_MAX_MEMBERS, f"ensemble_scores_sums: members must hold 2..{ENSEMBLE_MAX_MEMBERS} lists, got {M}"
    dev, n_lat = row_w.device, row_w.shape[0]
    n_lon = truth[0].shape[-1] if truth else 1
    lists = [(f"member {m}", fs) for m, fs in enumerate(members)] + [("truth", truth)]
    planes = _planes("ensemble_scores_sums", lists, dev, "row_w", n_lat, n_lon, like=-1)
    n = planes.n
    sums = torch.empty(n, 8, dtype=torch.float64, device=dev)
    hist = torch.empty(n, M + 2, dtype=torch.int64, device=dev)
    if n == 0:
        return sums, hist
    at = planes.upload()
    workspace = torch.empty(ensemble_scores_workspace_bytes(M, n, n_lat, n_lon), dtype=torch.uint8, device=dev)
    _launch(dev, "ensemble_scores", 0.0, "aurora_hip_ensemble_scores", at["member 0"], at["truth"], M, n, n_lat, n_lon,
            _ptr(row_w), _ptr(sums), _ptr(hist), _ptr(workspace))
    return sums, hist


# ---- quantile maps of an ensemble (aurora_hip_ensemble_quantiles) --------------------------------------------------------
QUANTILES_MAX = 8


def ensemble_quantiles(members: list[list[torch.Tensor]], truth: Optional[list[torch.Tensor]], q,
                       out: Optional[torch.Tensor] = None,
                       rank_out: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The quantile maps of include/aurora_hip.h for every plane of M members, and with `truth` the map of its rank among them,
    in ONE aurora_hip_ensemble_quantiles call (one launch): an (n_planes, Q, n_lat, n_lon) fp32 tensor and an (n_planes, n_lat,
    n_lon) int8 tensor (None without a truth) on the device.

    members: M lists (2 <= M <= 64), each like `truth`: fp32 (..., n_lat, n_lon) tensors on one device with row-major
    contiguous planes (any leading strides, any 4-byte plane alignment) and the same leading shapes; truth: one such list or
    None; q: 1 to 8 finite values in [0, 1] on the HOST (the library forms the indices and passes them by value); out / rank_out:
    contiguous tensors of the result's shape and dtype on that device to write into (any 4-byte / 1-byte alignment), or None
    to allocate them.  The plane-pointer table is cached by address as in `scores_sums`.  Nothing but the outputs is allocated
    and the host does not wait for the device."""
    M = len(members)
    assert 2 <= M <= ENSEMBLE_MAX_MEMBERS, f"ensemble_quantiles: members must hold 2..{ENSEMBLE_MAX_MEMBERS} lists, got {M}"
    assert members[0], "ensemble_quantiles: no fields"
    qs = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    Q = qs.shape[0]
    assert 1 <= Q <= QUANTILES_MAX, f"ensemble_quantiles: 1..{QUANTILES_MAX} values of q, got {Q}"
    assert rank_out is None or truth is not None, "ensemble_quantiles: rank_out without a truth"
    dev, (n_lat, n_lon) = members[0][0].device, members[0][0].shape[-2:]
    lists = [(f"member {m}", fs) for m, fs in enumerate(members)] + [("truth", truth)]
    planes = _planes("ensemble_quantiles", lists, dev, "the first member", n_lat, n_lon)
    n = planes.n
    text = "{what} must be a contiguous {dtype} tensor of {shape} on the device of {anchor}"
    out, = _outputs("ensemble_quantiles", None if out is None else (out,), [((n, Q, n_lat, n_lon), torch.float32, "out")], dev,
                    "the members", text)
    if truth is not None:
        rank_out, = _outputs("ensemble_quantiles", None if rank_out is None else (rank_out,),
                             [((n, n_lat, n_lon), torch.int8, "rank_out")], dev, "the members", text)
    at = planes.upload()
    moved = float(n * n_lat * n_lon * (4 * M + 4 * Q + (5 if truth is not None else 0)))
    _launch(dev, "ensemble_quantiles", moved, "aurora_hip_ensemble_quantiles", at["member 0"], at["truth"], M, n, n_lat, n_lon,
            qs.ctypes.data, Q, _ptr(out), _ptr(rank_out))
    return out, rank_out


# ---- event probabilities of an ensemble (aurora_hip_probability_scores) -----------------------------------------------
def probability_rows(members: list[list[torch.Tensor]], truth: list[torch.Tensor], thresholds: torch.Tensor,
                     below: bool = False) -> torch.Tensor:
    """The integer table of include/aurora_hip.h -- per row of every plane, threshold and (event observed o, k of M members
    forecasting it) the number of valid points -- in ONE aurora_hip_probability_scores call: an (n_planes, n_lat, T, 2, M + 1)
    int32 tensor on the device.

    members: M lists (2 <= M <= 64), each like `truth`: fp32 (..., n_lat, n_lon) tensors on one device with row-major
    contiguous planes (any leading strides, any 4-byte plane alignment) and the leading shapes of `truth`; thresholds:
    contiguous (n_planes, T) fp32 on that device (NaN: no event).  The plane-pointer table is cached by address as in
    `scores_sums`.  Nothing but the result is allocated and the host does not wait for the device."""
    _operand("probability_rows", "thresholds", thresholds, torch.float32, "(n_planes, T) fp32 matrix", dim=2)
    dev, (n_thr_planes, T) = thresholds.device, thresholds.shape
    M = len(members)
    assert 2 <= M <= ENSEMBLE_MAX_MEMBERS, f"probability_rows: members must hold 2..{ENSEMBLE_MAX_MEMBERS} lists, got {M}"
    assert 1 <= T <= EVENT_MAX_THRESHOLDS, f"probability_rows: 1..{EVENT_MAX_THRESHOLDS} thresholds, got {T}"
    assert truth and all(len(fs) == len(truth) for fs in members), "probability_rows: the lists differ in length or are empty"
    n_lat, n_lon = truth[0].shape[-2:]
    lists = [(f"member {m}", fs) for m, fs in enumerate(members)] + [("truth", truth)]
    planes = _planes("probability_rows", lists, dev, "thresholds", n_lat, n_lon, like=-1)
    n = planes.n
    assert n == n_thr_planes, f"probability_rows: {n} planes but thresholds for {n_thr_planes}"
    rows = torch.empty(n, n_lat, T, 2, M + 1, dtype=torch.int32, device=dev)
    if n == 0:
        return rows
    at = planes.upload()
    _launch(dev, "probability_scores", 0.0, "aurora_hip_probability_scores", at["member 0"], at["truth"], M, n, n_lat, n_lon,
            _ptr(thresholds), T, 1 if below else 0, _ptr(rows))
    return rows


# ---- zonal power spectra (aurora_hip_spectra) -------------------------------------------------------------------------
SPECTRA_MAX_BANDS, SPECTRA_MAX_LON = 8, 4096


def spectra_twiddle(n_lon: int, device: torch.device) -> torch.Tensor:
    """(n_lon, 2) fp64 on `device`: cos(2 pi m / n_lon), sin(2 pi m / n_lon), computed on the host in fp64 and kept per
    (n_lon, device)."""
    def make():
        a = 2.0 * np.pi * np.arange(n_lon, dtype=np.float64) / n_lon
        return np.stack([np.cos(a), np.sin(a)], axis=1)

    return _twiddles.get((int(n_lon),), device, make,
                         "spectra_power: call once for this n_lon before capturing a graph (the twiddle table is "
                         "uploaded on the first call, which a captured graph cannot replay)")


def spectra_workspace_bytes(n_planes: int, n_lat: int, n_lon: int, n_bands: int, has_truth: bool) -> int:
    return int(load().aurora_hip_spectra_workspace_bytes(n_planes, n_lat, n_lon, n_bands, 1 if has_truth else 0))


def spectra_power(pred: list[torch.Tensor], truth: Optional[list[torch.Tensor]],
                  band_w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Band-mean zonal power spectra (include/aurora_hip.h) of every plane of `pred` (and of the same plane of `truth` and of
    pred - truth, unless `truth` is None), in ONE aurora_hip_spectra call: an (n_planes, 1 or 3, n_bands, n_lon // 2 + 1)
    fp64 tensor and the (n_planes, n_bands) int64 counts of valid rows, on the device.

    pred / truth: lists of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading
    strides, any 4-byte plane alignment), the same leading shapes in each list; band_w: (n_bands, n_lat) fp64 on that
    device, the row weight inside the band and 0 outside.  The plane-pointer table is cached by address as in `scores_sums`,
    the twiddle table per n_lon; the only temporary is the workspace of partials.  The host does not wait for the device."""
    _operand("spectra_power", "band_w", band_w, torch.float64, "(n_bands, n_lat) fp64 matrix", dim=2)
    dev, (n_bands, n_lat) = band_w.device, band_w.shape
    assert 1 <= n_bands <= SPECTRA_MAX_BANDS, f"spectra_power: 1..{SPECTRA_MAX_BANDS} bands, got {n_bands}"
    n_lon = pred[0].shape[-1] if pred else 2
    assert 2 <= n_lon <= SPECTRA_MAX_LON, f"spectra_power: n_lon must be in 2..{SPECTRA_MAX_LON}, got {n_lon}"
    planes = _planes("spectra_power", [("prediction", pred), ("truth", truth)], dev, "band_w", n_lat, n_lon)
    n, n_lists = planes.n, 1 if truth is None else 2
    F, K = n_lists * 2 - 1, n_lon // 2 + 1
    power = torch.empty(n, F, n_bands, K, dtype=torch.float64, device=dev)
    rows = torch.empty(n, n_bands, dtype=torch.int64, device=dev)
    if n == 0:
        return power, rows
    at = planes.upload()
    twiddle = spectra_twiddle(n_lon, dev)
    nbytes = spectra_workspace_bytes(n, n_lat, n_lon, n_bands, truth is not None)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # (from torch's caching allocator: no hipMalloc warm)
    _launch(dev, "spectra", 2.0 * (n_lists * n * n_lat) * K * (2 * K),   # folded transform: K products per output
            "aurora_hip_spectra", at["prediction"], at["truth"], n, n_lat, n_lon, n_bands, _ptr(band_w), _ptr(twiddle),
            _ptr(power), _ptr(rows), _ptr(workspace), nbytes)
    return power, rows


# ---- spherical-harmonic power spectra (aurora_hip_sphere_spectra) -----------------------------------------------------------
SPHERE_TABLE_CAP = 1 << 30


def sphere_spectra_workspace_bytes(n_planes: int, n_lat: int, n_lon: int, lmax: int, has_truth: bool) -> int:
    return int(load().aurora_hip_sphere_spectra_workspace_bytes(n_planes, n_lat, n_lon, lmax, 1 if has_truth else 0))


def sphere_spectra_power(pred: list[torch.Tensor], truth: Optional[list[torch.Tensor]], table: torch.Tensor, lmax: int,
                         pole_rows: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Power spectra by total wavenumber (include/aurora_hip.h) of every plane of `pred` (and of the same plane of `truth` and
    of pred - truth, unless `truth` is None), in ONE aurora_hip_sphere_spectra call: an (n_planes, 1 or 3, lmax + 1) fp64
    tensor, the (n_planes,) bool validity and the (n_planes,) int32 counts of dropped pole rows, on the device.

    pred / truth: lists of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading
    strides, any 4-byte plane alignment), the same leading shapes in each list; table: the packed analysis table,
    ((lmax + 1)(lmax + 2) / 2, n_lat) fp64 on that device; pole_rows: bit 0 -- row 0 is a pole, bit 1 -- the last row is one.
    The plane-pointer table is cached by address as in `scores_sums`, the twiddle table per n_lon; the only temporary is the
    workspace (`sphere_spectra_workspace_bytes`: 16 (lmax + 1) n_lat bytes per plane and input, plus the partial sums).  The
    host does not wait for the device."""
    lmax = int(lmax)
    assert lmax >= 0, f"sphere_spectra_power: lmax must be at least 0, got {lmax}"
    _operand("sphere_spectra_power", "table", table, torch.float64, "((lmax + 1)(lmax + 2) / 2, n_lat) fp64 matrix", dim=2)
    dev, (n_rows, n_lat) = table.device, table.shape
    assert n_rows == (lmax + 1) * (lmax + 2) // 2, \
        f"sphere_spectra_power: the table has {n_rows} rows, lmax = {lmax} needs {(lmax + 1) * (lmax + 2) // 2}"
    n_lon = pred[0].shape[-1] if pred else 2
    assert 2 <= n_lon <= SPECTRA_MAX_LON, f"sphere_spectra_power: n_lon must be in 2..{SPECTRA_MAX_LON}, got {n_lon}"
    assert lmax <= min((n_lat - 1) // 2, (n_lon - 1) // 2), \
        f"sphere_spectra_power: lmax = {lmax} is above min((n_lat - 1) // 2, (n_lon - 1) // 2) on a {n_lat} x {n_lon} grid"
    planes = _planes("sphere_spectra_power", [("prediction", pred), ("truth", truth)], dev, "table", n_lat, n_lon)
    n, F = planes.n, 1 if truth is None else 3
    power = torch.empty(n, F, lmax + 1, dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    dropped = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return power, valid.view(torch.bool), dropped
    at = planes.upload()
    twiddle = spectra_twiddle(n_lon, dev)
    nbytes = sphere_spectra_workspace_bytes(n, n_lat, n_lon, lmax, truth is not None)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # (from torch's caching allocator: no hipMalloc warm)
    K = n_lon // 2 + 1
    work = 2.0 * ((F + 1) // 2 * n * n_lat) * K * (2 * (lmax + 1)) + 2.0 * ((F + 1) // 2 * 2 * n) * n_lat * n_rows
    _launch(dev, "sphere_spectra", work, "aurora_hip_sphere_spectra", at["prediction"], at["truth"], n, n_lat, n_lon, lmax,
            int(pole_rows), _ptr(table), _ptr(twiddle), _ptr(power), _ptr(valid), _ptr(dropped), _ptr(workspace), nbytes)
    return power, valid.view(torch.bool), dropped


# ---- spherical-harmonic analysis and synthesis (aurora_hip_sphere_analysis, aurora_hip_sphere_synthesis) -------------------
def sphere_analysis_workspace_bytes(n_planes: int, n_lat: int, n_lon: int, lmax: int) -> int:
    return int(load().aurora_hip_sphere_analysis_workspace_bytes(n_planes, n_lat, n_lon, lmax))


def sphere_synthesis_workspace_bytes(n_planes: int, n_lat: int, n_lon: int, lmax: int) -> int:
    return int(load().aurora_hip_sphere_synthesis_workspace_bytes(n_planes, n_lat, n_lon, lmax))


def _sphere_table(fn: str, table: torch.Tensor, lmax: int) -> tuple:
    """`table` is a packed ((lmax + 1)(lmax + 2) / 2, n_lat) fp64 table on a device: (the device, n_lat)."""
    assert lmax >= 0, f"{fn}: lmax must be at least 0, got {lmax}"
    _operand(fn, "table", table, torch.float64, "((lmax + 1)(lmax + 2) / 2, n_lat) fp64 matrix", dim=2)
    n_rows, n_lat = table.shape
    assert n_rows == (lmax + 1) * (lmax + 2) // 2, f"{fn}: the table has {n_rows} rows, lmax = {lmax} needs {(lmax + 1) * (lmax + 2) // 2}"
    return table.device, n_lat


def sphere_analysis(fields: list[torch.Tensor], table: torch.Tensor, lmax: int,
                    pole_rows: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The spherical-harmonic coefficients (include/aurora_hip.h) of every plane of `fields`, in ONE aurora_hip_sphere_analysis
    call of two launches: an (n_planes, lmax + 1 [m], lmax + 1 [l]) complex128 tensor, 0 where l < m and NaN for an invalid
    plane, the (n_planes,) bool validity and the (n_planes,) int32 counts of dropped pole rows, on the device.

    fields: a list of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading strides, any
    4-byte plane alignment); table: the packed ANALYSIS table of `sphere_spectra_power`; pole_rows: as there.  The
    plane-pointer table is cached by address as in `scores_sums`, the twiddle table per n_lon; the only temporary is the
    workspace (`sphere_analysis_workspace_bytes`: 16 (lmax + 1) n_lat bytes per plane).  The host does not wait for the device."""
    lmax = int(lmax)
    dev, n_lat = _sphere_table("sphere_analysis", table, lmax)
    n_lon = fields[0].shape[-1] if fields else 2
    assert 2 <= n_lon <= SPECTRA_MAX_LON, f"sphere_analysis: n_lon must be in 2..{SPECTRA_MAX_LON}, got {n_lon}"
    assert lmax <= min((n_lat - 1) // 2, (n_lon - 1) // 2), \
        f"sphere_analysis: lmax = {lmax} is above min((n_lat - 1) // 2, (n_lon - 1) // 2) on a {n_lat} x {n_lon} grid"
    planes = _planes("sphere_analysis", [("field", fields)], dev, "table", n_lat, n_lon)
    n = planes.n
    coeff = torch.empty(n, lmax + 1, lmax + 1, 2, dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    dropped = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return torch.view_as_complex(coeff), valid.view(torch.bool), dropped
    at = planes.upload()
    twiddle = spectra_twiddle(n_lon, dev)
    nbytes = sphere_analysis_workspace_bytes(n, n_lat, n_lon, lmax)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # (from torch's caching allocator: no hipMalloc warm)
    K = n_lon // 2 + 1
    work = 2.0 * (n * n_lat) * K * (2 * (lmax + 1)) + 2.0 * (2 * n) * n_lat * table.shape[0]
    _launch(dev, "sphere_analysis", work, "aurora_hip_sphere_analysis", at["field"], n, n_lat, n_lon, lmax, int(pole_rows),
            _ptr(table), _ptr(twiddle), _ptr(coeff), _ptr(valid), _ptr(dropped), _ptr(workspace), nbytes)
    return torch.view_as_complex(coeff), valid.view(torch.bool), dropped


def sphere_synthesis(coeff: torch.Tensor, table: torch.Tensor, n_lon: int, valid: Optional[torch.Tensor] = None, *,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fields of the coefficients (include/aurora_hip.h), in ONE aurora_hip_sphere_synthesis call of two launches: an
    (n_planes, n_lat, n_lon) fp32 tensor on the device.

    coeff: a contiguous (n_planes, lmax + 1 [m], lmax + 1 [l]) complex128 tensor on a device (elements with l < m are not read);
    table: the packed SYNTHESIS table, ((lmax + 1)(lmax + 2) / 2, n_lat) fp64 on that device; valid: a contiguous (n_planes,)
    bool tensor there -- a plane whose entry is False comes out as NaN -- or None: every plane is synthesised; out: a
    contiguous fp32 tensor of the result's shape to write into (any 4-byte alignment), allocated when not given.  The twiddle
    table is kept per n_lon; the only temporary is the workspace (`sphere_synthesis_workspace_bytes`: 16 (lmax + 1) n_lat bytes
    per plane).  The host does not wait for the device."""
    assert coeff.is_cuda and coeff.dtype == torch.complex128 and coeff.dim() == 3 and coeff.shape[1] == coeff.shape[2] and \
        coeff.is_contiguous(), "sphere_synthesis: coeff must be a contiguous (n_planes, lmax + 1, lmax + 1) complex128 tensor on the device"
    n, lmax, n_lon = coeff.shape[0], coeff.shape[1] - 1, int(n_lon)
    dev, n_lat = _sphere_table("sphere_synthesis", table, lmax)
    assert coeff.device == dev, "sphere_synthesis: every tensor must be on the device of table"
    assert 2 <= n_lon <= SPECTRA_MAX_LON, f"sphere_synthesis: n_lon must be in 2..{SPECTRA_MAX_LON}, got {n_lon}"
    assert lmax <= min((n_lat - 1) // 2, (n_lon - 1) // 2), \
        f"sphere_synthesis: lmax = {lmax} is above min((n_lat - 1) // 2, (n_lon - 1) // 2) on a {n_lat} x {n_lon} grid"
    if valid is not None:
        _like("sphere_synthesis", "valid", valid, (n,), torch.bool, dev, "table")
    (out,) = _outputs("sphere_synthesis", None if out is None else (out,), (((n, n_lat, n_lon), torch.float32, "out"),), dev, "table")
    if n == 0:
        return out
    twiddle = spectra_twiddle(n_lon, dev)
    nbytes = sphere_synthesis_workspace_bytes(n, n_lat, n_lon, lmax)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # (from torch's caching allocator: no hipMalloc warm)
    work = 2.0 * (2 * n) * n_lat * table.shape[0] + 2.0 * (n * n_lat) * (n_lon // 2 + 1) * (2 * (lmax + 1))
    _launch(dev, "sphere_synthesis", work, "aurora_hip_sphere_synthesis", _ptr(coeff), None if valid is None else _ptr(valid), n,
            n_lat, n_lon, lmax, _ptr(table), _ptr(twiddle), _ptr(out), _ptr(workspace), nbytes)
    return out


# ---- events: contingency tables and fractions skill score (aurora_hip_event_scores) -----------------------------------
EVENT_MAX_THRESHOLDS, EVENT_MAX_SCALES, EVENT_MAX_SCALE, EVENT_MAX_LON = 8, 8, 63, 4096


def event_scores_workspace_bytes(n_planes: int, n_lat: int, n_lon: int, n_thresholds: int, n_scales: int) -> int:
    return int(load().aurora_hip_event_scores_workspace_bytes(n_planes, n_lat, n_lon, n_thresholds, n_scales))


def event_rowsums(pred: list[torch.Tensor], truth: list[torch.Tensor], thresholds: torch.Tensor, scales,
                  below: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """The integer row sums of include/aurora_hip.h (sum (cf - co)^2, sum cf^2, sum co^2 over the valid points of every row)
    of every plane of `pred` against the same plane of `truth`, for every threshold and window size, in ONE
    aurora_hip_event_scores call: an (n_planes, T, S, n_lat, 3) int64 tensor and the (n_planes, n_lat) int64 counts of valid
    points, on the device.

    pred / truth: lists of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading
    strides, any 4-byte plane alignment), the same leading shapes in each list; thresholds: contiguous (n_planes, T) fp32 on
    that device (NaN: no event); scales: odd, ascending, distinct window sizes starting with 1, each <= 63 and <= n_lon.
    The plane-pointer table is cached by address as in `scores_sums`.  Nothing of plane size is allocated and the host does
    not wait for the device."""
    _operand("event_rowsums", "thresholds", thresholds, torch.float32, "(n_planes, T) fp32 matrix", dim=2)
    dev, (n_thr_planes, T) = thresholds.device, thresholds.shape
    scales = [int(n) for n in scales]
    S = len(scales)
    assert 1 <= T <= EVENT_MAX_THRESHOLDS, f"event_rowsums: 1..{EVENT_MAX_THRESHOLDS} thresholds, got {T}"
    assert 1 <= S <= EVENT_MAX_SCALES, f"event_rowsums: 1..{EVENT_MAX_SCALES} scales, got {S}"
    assert len(truth) == len(pred) and pred, "event_rowsums: the lists differ in length or are empty"
    n_lat, n_lon = pred[0].shape[-2:]
    planes = _planes("event_rowsums", [("prediction", pred), ("truth", truth)], dev, "thresholds", n_lat, n_lon)
    n = planes.n
    assert n == n_thr_planes, f"event_rowsums: {n} planes but thresholds for {n_thr_planes}"
    rowsums = torch.empty(n, T, S, n_lat, 3, dtype=torch.int64, device=dev)
    valid = torch.empty(n, n_lat, dtype=torch.int64, device=dev)
    if n == 0:
        return rowsums, valid
    at = planes.upload()
    _launch(dev, "event_scores", 0.0, "aurora_hip_event_scores", at["prediction"], at["truth"], n, n_lat, n_lon,
            _ptr(thresholds), T, (c_int32 * S)(*scales), S, 1 if below else 0, _ptr(rowsums), _ptr(valid), None, 0)
    return rowsums, valid


# ---- conditional sums: the error sums per bin of the truth (aurora_hip_conditional_scores) ------------------------------
def conditional_scores_workspace_bytes(n_planes: int, n_lat: int, n_lon: int, n_edges: int) -> int:
    return int(load().aurora_hip_conditional_scores_workspace_bytes(n_planes, n_lat, n_lon, n_edges))


def conditional_sums(pred: list[torch.Tensor], truth: list[torch.Tensor], centre: Optional[list[torch.Tensor]],
                     scale: Optional[list[torch.Tensor]], edges: torch.Tensor, by_pred: bool, row_w: torch.Tensor) -> torch.Tensor:
    """The five sums of include/aurora_hip.h (count, w, w d, w d^2, w |d|) per bin of every plane of `pred` against the same
    plane of `truth`, binned by the rule there with the planes of `centre` and `scale` (each a list or None), as an
    (n_planes, E + 1, 5) fp64 tensor on the device, in ONE aurora_hip_conditional_scores call.

    pred / truth / centre / scale: lists of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes
    (any leading strides -- a leading stride of 0 repeats a plane's address, nothing is copied -- and any 4-byte plane
    alignment), the same leading shapes in each list; edges: contiguous (n_planes, E) fp32 on that device, 1 <= E <= 8 (NaN:
    no edge); row_w: (n_lat,) fp64 on that device.  The plane-pointer table is cached by address as in `scores_sums`.
    Nothing of plane size is allocated and the host does not wait for the device."""
    _operand("conditional_sums", "row_w", row_w, torch.float64, "fp64 vector", dim=1)
    _operand("conditional_sums", "edges", edges, torch.float32, "(n_planes, E) fp32 matrix", dim=2)
    dev, n_lat, (n_edge_planes, E) = row_w.device, row_w.shape[0], edges.shape
    assert edges.device == dev, "conditional_sums: every tensor must be on the device of row_w"
    assert 1 <= E <= EVENT_MAX_THRESHOLDS, f"conditional_sums: 1..{EVENT_MAX_THRESHOLDS} edges, got {E}"
    lists = [("prediction", pred), ("truth", truth), ("centre", centre), ("scale", scale)]
    n_lon = pred[0].shape[-1] if pred else 1
    planes = _planes("conditional_sums", lists, dev, "row_w", n_lat, n_lon)
    n = planes.n
    assert n == n_edge_planes, f"conditional_sums: {n} planes but edges for {n_edge_planes}"
    sums = torch.empty(n, E + 1, 5, dtype=torch.float64, device=dev)
    if n == 0:
        return sums
    at = planes.upload()
    workspace = torch.empty(conditional_scores_workspace_bytes(n, n_lat, n_lon, E), dtype=torch.uint8, device=dev)
    read = n * n_lat * n_lon * 4 * sum(fs is not None for _, fs in lists)   # bytes
    _launch(dev, "conditional_scores", float(read), "aurora_hip_conditional_scores", at["prediction"], at["truth"],
            at["centre"], at["scale"], n, n_lat, n_lon, _ptr(edges), E, 1 if by_pred else 0, _ptr(row_w), _ptr(sums),
            _ptr(workspace))
    return sums


# ---- region sums: the verification sums per region (aurora_hip_region_scores) --------------------------------------------
REGION_MAX_PER_CALL = 8


def region_scores_workspace_bytes(n_planes: int, n_lat: int, n_lon: int, n_regions: int) -> int:
    return int(load().aurora_hip_region_scores_workspace_bytes(n_planes, n_lat, n_lon, n_regions))


def region_sums(pred: list[torch.Tensor], truth: list[torch.Tensor], clim: Optional[list[torch.Tensor]], row_bits: torch.Tensor,
                col_bits: torch.Tensor, mask_bits: Optional[torch.Tensor], n_regions: int, row_w: torch.Tensor) -> torch.Tensor:
    """The eight sums of `scores_sums` per region of every plane of `pred` against the same plane of `truth` (and of `clim`, or
    None), as an (n_planes, n_regions, 8) fp64 tensor on the device, in ONE aurora_hip_region_scores call.  A point belongs to
    region r where bit r of row_bits[row] & col_bits[col] & mask_bits[row, col] is set (mask_bits None: every bit set).

    pred / truth / clim: as in `scores_sums`; row_bits: (n_lat,) uint8, col_bits: (n_lon,) uint8, mask_bits: None or
    (n_lat, n_lon) uint8, contiguous, on that device, any alignment; 1 <= n_regions <= 8; row_w: (n_lat,) fp64 on that device.
    The plane-pointer table is cached by address as in `scores_sums`.  Nothing of plane size is allocated and the host does
    not wait for the device."""
    _operand("region_sums", "row_w", row_w, torch.float64, "fp64 vector", dim=1)
    dev, n_lat = row_w.device, row_w.shape[0]
    assert 1 <= n_regions <= REGION_MAX_PER_CALL, f"region_sums: 1..{REGION_MAX_PER_CALL} regions per call, got {n_regions}"
    n_lon = pred[0].shape[-1] if pred else col_bits.shape[0]
    for what, t, shape in (("row_bits", row_bits, (n_lat,)), ("col_bits", col_bits, (n_lon,)), ("mask_bits", mask_bits, (n_lat, n_lon))):
        if t is not None:
            assert t.dtype == torch.uint8 and tuple(t.shape) == shape and t.is_contiguous(), \
                f"region_sums: {what} must be a contiguous uint8 tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}"
            assert t.device == dev, "region_sums: every tensor must be on the device of row_w"
    planes = _planes("region_sums", [("prediction", pred), ("truth", truth), ("climatology", clim)], dev, "row_w", n_lat, n_lon)
    n = planes.n
    sums = torch.empty(n, n_regions, 8, dtype=torch.float64, device=dev)
    if n == 0:
        return sums
    at = planes.upload()
    workspace = torch.empty(region_scores_workspace_bytes(n, n_lat, n_lon, n_regions), dtype=torch.uint8, device=dev)
    read = n * n_lat * n_lon * (4 * (2 if clim is None else 3) + (1 if mask_bits is not None else 0))
    _launch(dev, "region_scores", float(read),   # bytes read, were every row in some region
            "aurora_hip_region_scores", at["prediction"], at["truth"], at["climatology"], n, n_lat, n_lon, _ptr(row_bits),
            _ptr(col_bits), _ptr(mask_bits), n_regions, _ptr(row_w), _ptr(sums), _ptr(workspace))
    return sums


# ---- threshold objects: connected components and their table (aurora_hip_objects) ------------------------------------------
OBJECT_MAX_THRESHOLDS, OBJECT_MAX_LON, OBJECT_COLUMNS, OBJECT_MAX_POINTS = 8, 4096, 10, 2 ** 31 - 2


def objects_workspace_bytes(n_planes: int, n_lat: int, n_lon: int, n_thresholds: int) -> int:
    return int(load().aurora_hip_objects_workspace_bytes(n_planes, n_lat, n_lon, n_thresholds))


def object_labels(fields: list[torch.Tensor], thresholds: torch.Tensor, unit: torch.Tensor, below: bool = False,
                  connectivity: int = 8, wrap: bool = False, max_objects: int = 4096, *, out=None,
                  workspace: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The objects (include/aurora_hip.h) of every plane of `fields` for every threshold, in ONE aurora_hip_objects call:
    labels (n_planes, T, n_lat, n_lon) int32, count (n_planes, T) int32 and table (n_planes, T, max_objects, 10) int64, on the
    device.

    fields: a list of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading strides,
    any 4-byte plane alignment); thresholds: contiguous (n_planes, T) fp32 on that device (NaN: no event); unit: contiguous
    (n_lat,) int64 on that device, the area units of the rows.  out: (labels, count, table) to write into, contiguous and of
    those shapes; workspace: a uint8 tensor of at least `objects_workspace_bytes` bytes -- both are allocated when not given
    (the workspace is plane-sized: 4 bytes per point and threshold).  The plane-pointer table is cached by address as in
    `scores_sums`.  The host does not wait for the device."""
    _operand("object_labels", "thresholds", thresholds, torch.float32, "(n_planes, T) fp32 matrix", dim=2)
    dev, (n_thr_planes, T) = thresholds.device, thresholds.shape
    assert 1 <= T <= OBJECT_MAX_THRESHOLDS, f"object_labels: 1..{OBJECT_MAX_THRESHOLDS} thresholds, got {T}"
    assert fields, "object_labels: the list of fields is empty"
    n_lat, n_lon = fields[0].shape[-2:]
    _operand("object_labels", "unit", unit, torch.int64, "(n_lat,) int64 vector", dev=dev, anchor="thresholds", shape=(n_lat,))
    max_objects = int(max_objects)
    planes = _planes("object_labels", [("field", fields)], dev, "thresholds", n_lat, n_lon)
    n = planes.n
    assert n == n_thr_planes, f"object_labels: {n} planes but thresholds for {n_thr_planes}"
    labels, count, table = _outputs("object_labels", out, (((n, T, n_lat, n_lon), torch.int32, "labels"), ((n, T), torch.int32, "count"),
                                                           ((n, T, max(max_objects, 0), OBJECT_COLUMNS), torch.int64, "table")),
                                    dev, "thresholds")
    if n == 0:
        return labels, count, table
    at = planes.upload()
    workspace = _workspace("object_labels", workspace, dev, "thresholds", objects_workspace_bytes, n, n_lat, n_lon, T)
    _launch(dev, "objects", 0.0, "aurora_hip_objects", at["field"], n, n_lat, n_lon, _ptr(thresholds), T, _ptr(unit),
            1 if below else 0, int(connectivity), 1 if wrap else 0, max_objects, _ptr(labels), _ptr(count), _ptr(table),
            _ptr(workspace), workspace.numel())
    return labels, count, table


# ---- overlap pairs of two label maps (aurora_hip_object_matches) -----------------------------------------------------------------
OBJECT_MAX_PAIRS, OBJECT_PAIR_COLUMNS = 8192, 4


def object_matches_workspace_bytes(n_items: int, max_pairs: int) -> int:
    return int(load().aurora_hip_object_matches_workspace_bytes(n_items, max_pairs))


def object_pairs(labels_a: torch.Tensor, labels_b: torch.Tensor, unit: torch.Tensor, max_objects_a: int, max_objects_b: int,
                 max_pairs: int, *, out=None, workspace: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The overlap pairs (include/aurora_hip.h) of every item of two stacks of label maps, in ONE aurora_hip_object_matches call:
    pairs (*lead, max_pairs, 4) int64 -- ka, kb, points, area units, ascending, zero past count -- and count (*lead) int32, -1
    where an item has more than max_pairs, on the device.

    labels_a, labels_b: contiguous int32 (*lead, n_lat, n_lon) tensors of one shape on one device (any 4-byte alignment), e.g.
    the labels of `object_labels`; they need not be connected; unit: contiguous (n_lat,) int64 on that device, the area units of
    the rows.  out: (pairs, count) to write into, contiguous and of those shapes; workspace: a uint8 tensor of at least
    `object_matches_workspace_bytes` bytes -- both are allocated when not given (the workspace holds hash tables only: 48 to 96
    bytes per pair of max_pairs and item).  The host does not wait for the device."""
    dev, (n_lat, n_lon), lead = _label_maps("object_pairs", "labels_a", labels_a)
    assert labels_b.device == dev and labels_b.dtype == torch.int32 and labels_b.shape == labels_a.shape and labels_b.is_contiguous(), \
        f"object_pairs: labels_b must be a contiguous int32 tensor of shape {tuple(labels_a.shape)} on the device of labels_a"
    _operand("object_pairs", "unit", unit, torch.int64, "(n_lat,) int64 vector", dev=dev, anchor="labels_a", shape=(n_lat,))
    max_objects_a, max_objects_b, max_pairs = int(max_objects_a), int(max_objects_b), int(max_pairs)
    n = int(np.prod(lead, dtype=np.int64))
    pairs, count = _outputs("object_pairs", out, (((*lead, max(max_pairs, 0), OBJECT_PAIR_COLUMNS), torch.int64, "pairs"),
                                                  (lead, torch.int32, "count")), dev, "labels_a")
    if n == 0:
        return pairs, count
    workspace = _workspace("object_pairs", workspace, dev, "labels_a", object_matches_workspace_bytes, n, max_pairs)
    _launch(dev, "object_matches", float(8 * n * n_lat * n_lon),   # bytes read: both maps once
            "aurora_hip_object_matches", _ptr(labels_a), _ptr(labels_b), n, n_lat, n_lon, _ptr(unit), max_objects_a, max_objects_b,
            max_pairs, _ptr(count), _ptr(pairs), _ptr(workspace), workspace.numel())
    return pairs, count


# ---- the nearest event of every point, the separations of objects (aurora_hip_nearest_event, aurora_hip_object_separations) ------
NEAREST_MAX_LON, SEPARATION_COLUMNS = 4096, 3


def nearest_event_workspace_bytes(n_items: int, n_lat: int, n_lon: int) -> int:
    return int(load().aurora_hip_nearest_event_workspace_bytes(n_items, n_lat, n_lon))


def nearest_event_maps(labels: torch.Tensor, tables: torch.Tensor, wrap: bool, key_max: float = float("inf"), *, out=None,
                       workspace: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The nearest event (include/aurora_hip.h) of every point of a stack of label maps, in ONE aurora_hip_nearest_event call:
    index (*lead, n_lat, n_lon) int32 -- the flat index of the nearest point with label > 0, -1 for none -- and key, the same
    shape in fp64 -- 1 - cos(angle), +inf for none -- on the device.

    labels: a contiguous int32 (*lead, n_lat, n_lon) tensor on the device (any 4-byte alignment); tables: contiguous
    (2 n_lat + n_lon,) fp64 on that device: sin(lat), max(cos(lat), 0), cos(d dlon); key_max: candidates beyond it are ignored
    (a HOST number, passed by value).  out: (index, key) to write into, contiguous and of those shapes; workspace: a uint8 tensor
    of at least `nearest_event_workspace_bytes` bytes -- both are allocated when not given (the workspace is plane-sized: 2 bytes
    per point).  The host does not wait for the device."""
    dev, (n_lat, n_lon), lead = _label_maps("nearest_event_maps", "labels", labels)
    _operand("nearest_event_maps", "tables", tables, torch.float64, "(2 n_lat + n_lon,) fp64 vector", dev=dev, anchor="labels",
             shape=(2 * n_lat + n_lon,))
    n = int(np.prod(lead, dtype=np.int64))
    index, key = _outputs("nearest_event_maps", out, ((labels.shape, torch.int32, "index"), (labels.shape, torch.float64, "key")),
                          dev, "labels")
    if n == 0:
        return index, key
    workspace = _workspace("nearest_event_maps", workspace, dev, "labels", nearest_event_workspace_bytes, n, n_lat, n_lon)
    _launch(dev, "nearest_event", float(16 * n * n_lat * n_lon),   # bytes: the map read once, the two maps written
            "aurora_hip_nearest_event", _ptr(labels), n, n_lat, n_lon, _ptr(tables), 1 if wrap else 0, float(key_max), _ptr(index),
            _ptr(key), _ptr(workspace), workspace.numel())
    return index, key


def object_separation_table(labels_a: torch.Tensor, key: torch.Tensor, index: torch.Tensor, count_a: torch.Tensor,
                            max_objects: int, *, out=None) -> tuple[torch.Tensor, torch.Tensor]:
    """The separations (include/aurora_hip.h) of the objects of `labels_a` from the events whose nearest-event maps are `key` and
    `index`, in ONE aurora_hip_object_separations call: table (*lead, max_objects, 3) int64 -- key bits, a_point, b_point -- and
    hausdorff (*lead) int64, the greatest key of the item's events as bits, on the device.

    labels_a, index: contiguous int32 (*lead, n_lat, n_lon) on one device; key: contiguous fp64 of that shape; count_a:
    contiguous int32 (*lead).  out: (table, hausdorff) to write into.  The host does not wait for the device."""
    dev, (n_lat, n_lon), lead = _label_maps("object_separation_table", "labels_a", labels_a)
    for t, d, s, what in ((key, torch.float64, labels_a.shape, "key"), (index, torch.int32, labels_a.shape, "index"),
                          (count_a, torch.int32, lead, "count_a")):
        _like("object_separation_table", what, t, s, d, dev, "labels_a")
    max_objects = int(max_objects)
    n = int(np.prod(lead, dtype=np.int64))
    table, hausdorff = _outputs("object_separation_table", out,
                                (((*lead, max(max_objects, 0), SEPARATION_COLUMNS), torch.int64, "table"), (lead, torch.int64, "hausdorff")),
                                dev, "labels_a", "{what} must be a contiguous int64 tensor of shape {shape} on the device of {anchor}")
    if n == 0:
        return table, hausdorff
    _launch(dev, "object_separations", float(32 * n * n_lat * n_lon),   # bytes: label, key and index read twice
            "aurora_hip_object_separations", _ptr(labels_a), _ptr(key), _ptr(index), _ptr(count_a), n, n_lat, n_lon, max_objects,
            _ptr(table), _ptr(hausdorff))
    return table, hausdorff


# ---- fields smoothed over a great-circle disc (aurora_hip_smooth) -----------------------------------------------------------------
SMOOTH_MAX_ROWS = 255
SMOOTH_WORKSPACE_CAP = 128 << 20   # bytes of prefix tables in flight: inside the 256 MiB Infinity Cache


def smooth_workspace_bytes(n_planes: int, n_lat: int, n_lon: int) -> int:
    return int(load().aurora_hip_smooth_workspace_bytes(n_planes, n_lat, n_lon))


def smooth_planes(fields: list[torch.Tensor], rows: torch.Tensor, w: torch.Tensor, wrap: bool, min_valid: float = 0.5,
                  keep_mask: bool = True, *, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                  workspace_cap: int = SMOOTH_WORKSPACE_CAP) -> torch.Tensor:
    """Every plane of `fields` smoothed over the disc of the table (include/aurora_hip.h), as an (n_planes, n_lat, n_lon) fp32
    tensor on the device, by aurora_hip_smooth calls (two launches each) over as many planes at a time as keep the workspace within `workspace_cap` bytes,
    at least one.

    fields: a list of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading strides, any
    4-byte plane alignment); out: a contiguous tensor of that shape to write into (it must not overlap a field), allocated when
    not given.  rows: the contiguous
    int32 vector [row_lo (n_lat) | row_count (n_lat) | half (n_lat x max_rows)] of `aurora_amd.smooth.disc_table` on that device;
    w: contiguous (n_lat,) fp64.  workspace: a uint8 tensor to use for the prefix tables, of at least
    `smooth_workspace_bytes(1, n_lat, n_lon)` bytes, or None: one of at most `workspace_cap` bytes is allocated.  The workspace
    is PLANE-SIZED: 12 bytes per point (and per row one entry more) of the planes in flight.  A plane's bytes do not depend on
    how the planes are divided.  The plane-pointer table is cached by address as in `scores_sums`.  The host does not wait for
    the device."""
    assert fields, "smooth_planes: the list of fields is empty"
    dev, (n_lat, n_lon) = fields[0].device, fields[0].shape[-2:]
    _operand("smooth_planes", "w", w, torch.float64, "(n_lat,) fp64 vector", dev=dev, anchor="the fields", shape=(n_lat,))
    _operand("smooth_planes", "rows", rows, torch.int32, "int32 vector", dev=dev, anchor="the fields", dim=1)
    max_rows = rows.numel() // n_lat - 2
    assert rows.numel() == n_lat * (2 + max_rows) and 1 <= max_rows <= SMOOTH_MAX_ROWS, \
        f"smooth_planes: rows holds {rows.numel()} entries, which is no table of 1..{SMOOTH_MAX_ROWS} source rows for {n_lat} latitudes"
    planes = _planes("smooth_planes", [("field", fields)], dev, "the first field", n_lat, n_lon)
    n = planes.n
    (out,) = _outputs("smooth_planes", None if out is None else (out,), (((n, n_lat, n_lon), torch.float32, "out"),), dev, "the fields")
    if n == 0:
        return out
    one = smooth_workspace_bytes(1, n_lat, n_lon)
    assert one > 0, f"smooth_planes: a plane of {n_lat} x {n_lon} points is too large"
    if workspace is None:
        chunk = min(n, max(1, int(workspace_cap) // one))
        workspace = torch.empty(smooth_workspace_bytes(chunk, n_lat, n_lon), dtype=torch.uint8, device=dev)
    else:
        workspace = _workspace("smooth_planes", workspace, dev, "the fields", smooth_workspace_bytes, 1, n_lat, n_lon)
        chunk = min(n, workspace.numel() // one)
        assert chunk >= 1, f"smooth_planes: the workspace has {workspace.numel()} bytes, a plane needs {one}"
    at = planes.upload()
    base = rows.data_ptr()
    for first in range(0, n, chunk):                            # on one stream: the next chunk reuses the workspace
        m = min(chunk, n - first)
        _launch(dev, "smooth", float(m * n_lat * n_lon * 8), "aurora_hip_smooth", at["field"] + 8 * first,
                out.data_ptr() + 4 * first * n_lat * n_lon, m,
                n_lat, n_lon, base, base + 4 * n_lat, base + 8 * n_lat, max_rows, _ptr(w), 1 if wrap else 0, float(min_valid),
                1 if keep_mask else 0, _ptr(workspace), workspace.numel())
    return out


# ---- local extrema over a great-circle disc (aurora_hip_extrema) --------------------------------------------------------------------
EXTREMA_MAX_LON, EXTREMA_MAX_POINTS, EXTREMA_COLUMNS = 4096, 65536, 2


def extrema_workspace_bytes(n_planes: int, n_lat: int, n_lon: int) -> int:
    return int(load().aurora_hip_extrema_workspace_bytes(n_planes, n_lat, n_lon))


def extrema_planes(fields: list[torch.Tensor], rows: torch.Tensor, wrap: bool, is_max: bool = False, max_points: int = 4096, *,
                   out=None, workspace: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The extreme point of the disc of every point of every plane of `fields` and the extrema of every plane
    (include/aurora_hip.h), in ONE aurora_hip_extrema call (four launches): index (n_planes, n_lat, n_lon) int32, filtered, the
    same shape in fp32, table (n_planes, max_points, 2) int64 and count (n_planes,) int32, on the device.

    fields: a list of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading strides, any
    4-byte plane alignment); rows: the contiguous int32 vector [row_lo (n_lat) | row_count (n_lat) | half (n_lat x max_rows)]
    of `aurora_amd.smooth.disc_table` on that device, the one `smooth_planes` takes.  out: (index, filtered, table, count) to
    write into, contiguous and of those shapes (they must not overlap a field); workspace: a uint8 tensor of at least
    `extrema_workspace_bytes` bytes -- both are allocated when not given (the workspace is NOT plane-sized: 16 bytes per row of
    every plane).  The plane-pointer table is cached by address as in `scores_sums`.  The host does not wait for the device."""
    assert fields, "extrema_planes: the list of fields is empty"
    dev, (n_lat, n_lon) = fields[0].device, fields[0].shape[-2:]
    assert 1 <= n_lon <= EXTREMA_MAX_LON, f"extrema_planes: n_lon must be in 1..{EXTREMA_MAX_LON}, got {n_lon}"
    _operand("extrema_planes", "rows", rows, torch.int32, "int32 vector", dev=dev, anchor="the fields", dim=1)
    max_rows = rows.numel() // n_lat - 2
    assert rows.numel() == n_lat * (2 + max_rows) and 1 <= max_rows <= SMOOTH_MAX_ROWS, \
        f"extrema_planes: rows holds {rows.numel()} entries, which is no table of 1..{SMOOTH_MAX_ROWS} source rows for {n_lat} latitudes"
    max_points = int(max_points)
    planes = _planes("extrema_planes", [("field", fields)], dev, "the first field", n_lat, n_lon)
    n = planes.n
    index, filtered, table, count = _outputs(
        "extrema_planes", out, (((n, n_lat, n_lon), torch.int32, "index"), ((n, n_lat, n_lon), torch.float32, "filtered"),
                                ((n, max(max_points, 0), EXTREMA_COLUMNS), torch.int64, "table"), ((n,), torch.int32, "count")),
        dev, "the fields")
    if n == 0:
        return index, filtered, table, count
    at = planes.upload()
    workspace = _workspace("extrema_planes", workspace, dev, "the fields", extrema_workspace_bytes, n, n_lat, n_lon)
    base = rows.data_ptr()
    _launch(dev, "extrema", float(12 * n * n_lat * n_lon),   # bytes: the planes read once, the two maps written
            "aurora_hip_extrema", at["field"], _ptr(index), _ptr(filtered), _ptr(table), _ptr(count), n, n_lat, n_lon, base,
            base + 4 * n_lat, base + 8 * n_lat, max_rows, 1 if wrap else 0, 1 if is_max else 0, max_points, _ptr(workspace),
            workspace.numel())
    return index, filtered, table, count


# ---- the closed-contour test of local extrema (aurora_hip_closed_contours) ----------------------------------------------------------
CONTOUR_MAX_DELTAS, CONTOUR_COLUMNS, CONTOUR_MAX_WORDS = 8, 2, 65
CONTOUR_LDS_BUDGET = 156 * 1024    # bytes of the three bitmaps of a workgroup: kContourLdsBudget of aurora_amd/csrc/contour_fill.h


def contour_lds_bytes(max_rows: int, max_words: int) -> int:
    """The LDS of the three bitmaps for windows of up to `max_rows` source rows and `max_words` words a row."""
    return 24 * (int(max_rows) + 2) * int(max_words)


def closed_contours_planes(fields: list[torch.Tensor], table: torch.Tensor, count: torch.Tensor, deltas: torch.Tensor,
                           rows: torch.Tensor, max_words: int, wrap: bool, is_max: bool = False, connectivity: int = 8, *,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The closed-contour test (include/aurora_hip.h) of every candidate of every plane of `fields` for every delta, in ONE
    aurora_hip_closed_contours call (one launch): (n_planes, T, max_points, 2) int32 on the device -- points, exits.

    fields: a list of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading strides, any
    4-byte plane alignment); table: contiguous (n_planes, max_points, 2) int64 and count: contiguous (n_planes,) int32 on that
    device, those of `extrema_planes`; deltas: contiguous (n_planes, T) fp32 on that device (NaN: none); rows: the contiguous
    int32 vector [row_lo (n_lat) | row_count (n_lat) | half (n_lat x max_rows)] of `aurora_amd.smooth.disc_table` on that
    device, the one `smooth_planes` takes; max_words: the most 64-column words a row of any candidate's window has
    (`aurora_amd.contours.window_words`).  out: the tensor to write into, contiguous and of that shape (it must not overlap an
    input), allocated when not given.  There is no workspace: the bitmaps live in LDS, `contour_lds_bytes(max_rows, max_words)`
    bytes a workgroup, at most CONTOUR_LDS_BUDGET.  The plane-pointer table is cached by address as in `scores_sums`.  The host
    does not wait for the device."""
    assert fields, "closed_contours_planes: the list of fields is empty"
    dev, (n_lat, n_lon) = fields[0].device, fields[0].shape[-2:]
    assert 1 <= n_lon <= EXTREMA_MAX_LON, f"closed_contours_planes: n_lon must be in 1..{EXTREMA_MAX_LON}, got {n_lon}"
    _operand("closed_contours_planes", "rows", rows, torch.int32, "int32 vector", dev=dev, anchor="the fields", dim=1)
    max_rows = rows.numel() // n_lat - 2
    assert rows.numel() == n_lat * (2 + max_rows) and 1 <= max_rows <= SMOOTH_MAX_ROWS, \
        f"closed_contours_planes: rows holds {rows.numel()} entries, which is no table of 1..{SMOOTH_MAX_ROWS} source rows for {n_lat} latitudes"
    _operand("closed_contours_planes", "deltas", deltas, torch.float32, "(n_planes, T) fp32 matrix", dev=dev, anchor="the fields", dim=2)
    T = deltas.shape[1]
    assert 1 <= T <= CONTOUR_MAX_DELTAS, f"closed_contours_planes: 1..{CONTOUR_MAX_DELTAS} deltas, got {T}"
    planes = _planes("closed_contours_planes", [("field", fields)], dev, "the first field", n_lat, n_lon)
    n = planes.n
    assert n == deltas.shape[0], f"closed_contours_planes: {n} planes but deltas for {deltas.shape[0]}"
    _operand("closed_contours_planes", "table", table, torch.int64, "(n_planes, max_points, 2) int64 tensor", dev=dev,
             anchor="the fields", dim=3)
    max_points = table.shape[1]
    assert tuple(table.shape) == (n, max_points, EXTREMA_COLUMNS), \
        f"closed_contours_planes: table has shape {tuple(table.shape)}, not ({n}, max_points, {EXTREMA_COLUMNS})"
    _operand("closed_contours_planes", "count", count, torch.int32, "(n_planes,) int32 vector", dev=dev, anchor="the fields", shape=(n,))
    (out,) = _outputs("closed_contours_planes", None if out is None else (out,),
                      (((n, T, max_points, CONTOUR_COLUMNS), torch.int32, "out"),), dev, "the fields")
    if n == 0:
        return out
    at = planes.upload()
    base = rows.data_ptr()
    _launch(dev, "closed_contours", 0.0, "aurora_hip_closed_contours", at["field"], _ptr(table), _ptr(count), _ptr(deltas), _ptr(out),
            n, n_lat, n_lon, T, max_points, base, base + 4 * n_lat, base + 8 * n_lat, max_rows, int(max_words), 1 if wrap else 0,
            1 if is_max else 0, int(connectivity))
    return out


# ---- linking the extrema of two steps (aurora_hip_link_extrema) ----------------------------------------------------------------------
LINK_COLUMNS = 2


def _overlaps(x: torch.Tensor, y: torch.Tensor) -> bool:
    """Do two contiguous tensors share a byte?"""
    x0, y0 = x.data_ptr(), y.data_ptr()
    return x0 < y0 + y.numel() * y.element_size() and y0 < x0 + x.numel() * x.element_size()


def link_extrema_tables(table_a: torch.Tensor, count_a: torch.Tensor, keep_a: Optional[torch.Tensor], table_b: torch.Tensor,
                        count_b: torch.Tensor, keep_b: Optional[torch.Tensor], tables: torch.Tensor, n_lat: int, n_lon: int,
                        wrap: bool, key_max: float = float("inf"), *, out=None) -> tuple[torch.Tensor, torch.Tensor]:
    """The links (include/aurora_hip.h) between the rows of two stacks of extrema tables, in ONE aurora_hip_link_extrema call (one
    launch): forward (n_planes, Ma, 2) int64 -- key bits, row of b -- and backward (n_planes, Mb, 2) int64 -- key bits, row of a
    -- on the device; the bits of +inf and -1 for none.

    table_a: contiguous (n_planes, Ma, 2) int64 and count_a: contiguous (n_planes,) int32 on the device, those of
    `extrema_planes`; keep_a: None or a contiguous (n_planes, Ma) bool tensor; the same for b with its own Mb; tables: contiguous
    (2 n_lat + n_lon,) fp64 on that device, those of `nearest_event_maps`; key_max: pairs beyond it are ignored (a HOST number,
    passed by value).  out: (forward, backward) to write into, contiguous and of those shapes; they must not overlap each other
    or an input.  No workspace.  The host does not wait for the device."""
    fn = "link_extrema_tables"
    _operand(fn, "table_a", table_a, torch.int64, "(n_planes, max_points, 2) int64 tensor", dim=3)
    dev, n = table_a.device, table_a.shape[0]
    _operand(fn, "table_b", table_b, torch.int64, "(n_planes, max_points, 2) int64 tensor", dev=dev, anchor="table_a", dim=3)
    for what, t in (("table_a", table_a), ("table_b", table_b)):
        assert t.shape[0] == n and t.shape[2] == EXTREMA_COLUMNS and 1 <= t.shape[1] <= EXTREMA_MAX_POINTS, \
            f"{fn}: {what} has shape {tuple(t.shape)}, not ({n}, 1..{EXTREMA_MAX_POINTS}, {EXTREMA_COLUMNS})"
    ma, mb = table_a.shape[1], table_b.shape[1]
    _operand(fn, "count_a", count_a, torch.int32, "(n_planes,) int32 vector", dev=dev, anchor="table_a", shape=(n,))
    _operand(fn, "count_b", count_b, torch.int32, "(n_planes,) int32 vector", dev=dev, anchor="table_a", shape=(n,))
    for what, t, m in (("keep_a", keep_a, ma), ("keep_b", keep_b, mb)):
        if t is not None:
            _operand(fn, what, t, torch.bool, "(n_planes, max_points) bool matrix", dev=dev, anchor="table_a", shape=(n, m))
    n_lat, n_lon = int(n_lat), int(n_lon)
    assert 1 <= n_lon <= NEAREST_MAX_LON and n_lat >= 1, f"{fn}: n_lat must be at least 1 and n_lon in 1..{NEAREST_MAX_LON}, got {n_lat} and {n_lon}"
    _operand(fn, "tables", tables, torch.float64, "(2 n_lat + n_lon,) fp64 vector", dev=dev, anchor="table_a", shape=(2 * n_lat + n_lon,))
    forward, backward = _outputs(fn, out, (((n, ma, LINK_COLUMNS), torch.int64, "forward"), ((n, mb, LINK_COLUMNS), torch.int64, "backward")),
                                 dev, "table_a")
    if n == 0:
        return forward, backward
    inputs = [t for t in (table_a, count_a, keep_a, table_b, count_b, keep_b, tables) if t is not None]
    assert not _overlaps(forward, backward) and not any(_overlaps(o, t) for o in (forward, backward) for t in inputs), \
        f"{fn}: forward and backward must not overlap each other or an input"
    _launch(dev, "link_extrema", 0.0, "aurora_hip_link_extrema", _ptr(table_a), _ptr(count_a), _ptr(keep_a), ma, _ptr(table_b),
            _ptr(count_b), _ptr(keep_b), mb, n, _ptr(tables), n_lat, n_lon, 1 if wrap else 0, float(key_max), _ptr(forward),
            _ptr(backward))
    return forward, backward


# ---- spatial quantiles of planes (aurora_hip_field_quantiles) ------------------------------------------------------------------
def field_quantiles_workspace_bytes(n_planes: int, n_q: int) -> int:
    return int(load().aurora_hip_field_quantiles_workspace_bytes(n_planes, n_q))


def field_quantile_values(fields: list[torch.Tensor], q, unit: Optional[torch.Tensor] = None, *, out=None,
                          workspace: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The spatial quantiles (include/aurora_hip.h) of every plane of `fields`, in ONE aurora_hip_field_quantiles call: values
    (n_planes, Q) fp32, valid (n_planes,) int64 and total (n_planes,) int64, on the device.

    fields: a list of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any leading strides,
    any 4-byte plane alignment); q: 1 to 8 finite values in [0, 1] on the HOST (passed to the kernels by value); unit: contiguous
    (n_lat,) int64 on that device, the area units of the rows (kind = area), or None (kind = count).  out: (values, valid,
    total) to write into, contiguous and of those shapes; workspace: a uint8 tensor of at least
    `field_quantiles_workspace_bytes` bytes -- both are allocated when not given (the workspace holds histograms only).  The
    plane-pointer table is cached by address as in `scores_sums`.  The host does not wait for the device."""
    assert fields, "field_quantile_values: the list of fields is empty"
    qs = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    Q = qs.shape[0]
    assert 1 <= Q <= QUANTILES_MAX, f"field_quantile_values: 1..{QUANTILES_MAX} values of q, got {Q}"
    dev, (n_lat, n_lon) = fields[0].device, fields[0].shape[-2:]
    if unit is not None:
        _operand("field_quantile_values", "unit", unit, torch.int64, "(n_lat,) int64 vector", dev=dev, anchor="the fields", shape=(n_lat,))
    planes = _planes("field_quantile_values", [("field", fields)], dev, "the first field", n_lat, n_lon)
    n = planes.n
    values, valid, total = _outputs("field_quantile_values", out, (((n, Q), torch.float32, "values"), ((n,), torch.int64, "valid"),
                                                                   ((n,), torch.int64, "total")), dev, "the fields")
    if n == 0:
        return values, valid, total
    at = planes.upload()
    workspace = _workspace("field_quantile_values", workspace, dev, "the fields", field_quantiles_workspace_bytes, n, Q)
    _launch(dev, "field_quantiles", float(4 * n * n_lat * n_lon * 4), "aurora_hip_field_quantiles", at["field"], n, n_lat, n_lon,
            _ptr(unit), qs.ctypes.data, Q, _ptr(values), _ptr(valid), _ptr(total), _ptr(workspace), workspace.numel())
    return values, valid, total


# ---- per-point statistics over a sequence of planes (aurora_hip_field_stats_update) -----------------------------------
FIELD_STATS_MAX_SAMPLES, FIELD_STATS_MAX_THRESHOLDS = 64, 8
# state array -> (dtype, per threshold); include/aurora_hip.h has the meanings
FIELD_STATS_STATE = {"n": (torch.int32, False), "origin": (torch.float32, False), "s1": (torch.float64, False),
                     "s2": (torch.float64, False), "vmin": (torch.float32, False), "vmax": (torch.float32, False),
                     "argmin": (torch.int32, False), "argmax": (torch.int32, False), "exceed": (torch.int32, True),
                     "run": (torch.int32, True), "longest": (torch.int32, True)}


def field_stats_update(samples: list[list[torch.Tensor]], ref: Optional[list[torch.Tensor]],
                       second: Optional[list[list[Optional[torch.Tensor]]]], thresholds: Optional[torch.Tensor], below: bool,
                       sample_index: torch.Tensor, state: dict[str, torch.Tensor]) -> None:
    """Applies S samples of every plane, in order, to the per-point `state` (include/aurora_hip.h: count, origin, shifted
    sums, minimum / maximum and the sample that reached them, exceedances and run lengths), in ONE
    aurora_hip_field_stats_update call, and advances `sample_index` on the device.

    samples: S lists (1 <= S <= 64) of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous planes (any
    leading strides, any 4-byte plane alignment), the same leading shapes in each list; ref: one such list or None (v = x -
    r); second: S such lists or None, an entry None where a field has no second operand (x <- sqrt(x^2 + b^2) elsewhere);
    thresholds: contiguous (n_planes, T) fp32 on that device, T <= 8, or None; sample_index: one int64 on the device; state:
    the arrays of FIELD_STATS_STATE, contiguous (n_planes, n_points) -- (n_planes, T, n_points) per threshold --, zero before
    the first call.  The plane-pointer table is cached by address as in `scores_sums`.  Nothing is allocated and the host
    does not wait for the device."""
    S = len(samples)
    assert 1 <= S <= FIELD_STATS_MAX_SAMPLES, f"field_stats_update: 1..{FIELD_STATS_MAX_SAMPLES} samples a call, got {S}"
    assert samples[0], "field_stats_update: no fields"
    dev = sample_index.device
    assert sample_index.is_cuda and sample_index.dtype == torch.int64 and sample_index.numel() == 1, \
        "field_stats_update: sample_index must be one int64 on the device"
    n_lat, n_lon = samples[0][0].shape[-2:]
    lists = [(f"sample {s}", fs) for s, fs in enumerate(samples)] + [("reference", ref)]
    planes = _planes("field_stats_update", lists, dev, "sample_index", n_lat, n_lon)
    n = planes.n
    seconds = None
    if second is not None:
        assert len(second) == S and all(len(fs) == len(samples[0]) for fs in second), \
            "field_stats_update: the second operands differ from the samples in number"
        seconds = []
        for s, fs in enumerate(second):
            for v, p in zip(fs, samples[s]):
                if v is None:
                    seconds += [0] * (p.numel() // (n_lat * n_lon))
                    continue
                assert v.device == dev and v.shape == p.shape, "field_stats_update: a second operand differs from its sample"
                seconds += _plane_addresses("field_stats_update", [v], n_lat, n_lon, "second operand")
    planes.add("second", seconds)
    T = 0
    if thresholds is not None:
        _operand("field_stats_update", "thresholds", thresholds, torch.float32, f"({n}, T) fp32 matrix", dev=dev, dim=2,
                 shape=(n, *thresholds.shape[1:2]))
        T = thresholds.shape[1]
        assert T <= FIELD_STATS_MAX_THRESHOLDS, f"field_stats_update: at most {FIELD_STATS_MAX_THRESHOLDS} thresholds, got {T}"
    for name, (dt, per_thr) in FIELD_STATS_STATE.items():
        if per_thr and T == 0:
            continue
        t = state[name]
        want = (n, T, n_lat * n_lon) if per_thr else (n, n_lat * n_lon)
        assert t.device == dev and t.dtype == dt and t.is_contiguous() and t.numel() == int(np.prod(want)), \
            f"field_stats_update: state {name!r} must be contiguous {dt} of {want} on the device"
    if n == 0:
        return
    at = planes.upload()
    arrays = [_ptr(state[k]) if (T or not per_thr) else None for k, (_, per_thr) in FIELD_STATS_STATE.items()]
    _launch(dev, "field_stats", float(n * n_lat * n_lon * (4 * S + 2 * (36 + 12 * T))), "aurora_hip_field_stats_update",
            at["sample 0"], at["reference"], at["second"], S, n, n_lat * n_lon, _ptr(thresholds) if T else None, T,
            1 if below else 0, _ptr(sample_index), *arrays)


# ---- derived fields (aurora_hip_diagnostics) ----------------------------------------------------------------------------
DIAGNOSTICS_MAX_LEVELS = 64


def diagnostics(n_lat: int, n_lon: int, *, u: Optional[list[torch.Tensor]] = None, v: Optional[list[torch.Tensor]] = None,
                vo: Optional[list[torch.Tensor]] = None, div: Optional[list[torch.Tensor]] = None,
                ws: Optional[list[torch.Tensor]] = None, row_table: Optional[torch.Tensor] = None, L: float = 0.0,
                wrap: bool = False, q: Optional[list[torch.Tensor]] = None, col_u: Optional[list[torch.Tensor]] = None,
                col_v: Optional[list[torch.Tensor]] = None, tcwv: Optional[list[torch.Tensor]] = None,
                ivtu: Optional[list[torch.Tensor]] = None, ivtv: Optional[list[torch.Tensor]] = None,
                ivt: Optional[list[torch.Tensor]] = None, level_w: Optional[torch.Tensor] = None) -> None:
    """Vorticity, divergence and wind speed of the wind planes (u, v) into (vo, div, ws), and the vertical integrals of the
    columns (q, col_u, col_v) into (tcwv, ivtu, ivtv, ivt), in ONE aurora_hip_diagnostics call: one launch per group
    (include/aurora_hip.h has the arithmetic).

    Every argument but the tables is a list of fp32 (..., n_lat, n_lon) tensors on one device with row-major contiguous
    planes (any leading strides, any 4-byte plane alignment) or None: an output that is None is skipped (an entry None of
    vo, div or ws, given entry for entry with u, skips it for the planes of that entry), and u = None / q = None leaves
    the group out.  The planes of a list are counted in row-major order of the leading dimensions: a wind
    output holds as many planes as u, and q (col_u, col_v) holds C = len(level_w) planes for every plane of a column
    output, levels fastest.  row_table: contiguous (n_lat, 4) fp64 on the device (None for wind speed alone); level_w: (C,)
    fp64 on the device.  An output must not share memory with an input.  The plane-pointer table is cached by address as
    in `scores_sums`.  Nothing is allocated and the host does not wait for the device."""
    groups = (("u", u), ("v", v), ("vo", vo), ("div", div), ("ws", ws), ("q", q), ("col_u", col_u), ("col_v", col_v),
              ("tcwv", tcwv), ("ivtu", ivtu), ("ivtv", ivtv), ("ivt", ivt))
    tensors = [t for _, fs in groups if fs is not None for t in fs if t is not None]
    if not tensors:
        return
    dev = tensors[0].device
    assert all(t.device == dev for t in tensors), "diagnostics: every tensor must be on one device"
    if row_table is not None:
        _operand("diagnostics", "row_table", row_table, torch.float64, f"fp64 {(n_lat, 4)}", dev=dev, anchor="the fields", shape=(n_lat, 4))
    if level_w is not None:
        _operand("diagnostics", "level_w", level_w, torch.float64, "fp64 vector", dev=dev, anchor="the fields", dim=1)
    addr = {}
    for what, fs in groups:
        if fs is None:
            continue
        if what in ("vo", "div", "ws") and any(t is None for t in fs):   # an entry None: NULL for the planes of that u entry
            assert u is not None and len(fs) == len(u), f"diagnostics: {what} with None entries must have an entry per u entry"
            addr[what] = [a for t, like in zip(fs, u) for a in
                          ([0] * (like.numel() // (n_lat * n_lon)) if t is None else _plane_addresses("diagnostics", [t], n_lat, n_lon, what))]
        else:
            addr[what] = _plane_addresses("diagnostics", fs, n_lat, n_lon, what)
    n_wind, n_cols = len(addr.get("u", ())), 0
    C = 0 if level_w is None else level_w.shape[0]
    for what in ("v", "vo", "div", "ws"):
        assert what not in addr or len(addr[what]) == n_wind, f"diagnostics: {what} holds {len(addr[what])} planes, u {n_wind}"
    if q is not None:
        assert C >= 1 and len(addr["q"]) % C == 0, f"diagnostics: q holds {len(addr['q'])} planes, which is no multiple of the {C} level weights"
        n_cols = len(addr["q"]) // C
        for what in ("col_u", "col_v"):
            assert what not in addr or len(addr[what]) == n_cols * C, f"diagnostics: {what} holds {len(addr[what])} planes, q {n_cols * C}"
        for what in ("tcwv", "ivtu", "ivtv", "ivt"):
            assert what not in addr or len(addr[what]) == n_cols, f"diagnostics: {what} holds {len(addr[what])} planes for {n_cols} columns"
    if n_wind == 0 and n_cols == 0:
        return
    planes = _planes("diagnostics", [], dev)
    for what, addresses in addr.items():   # (in the order of `groups`)
        planes.add(what, addresses)
    at = planes.upload()
    moved = 4.0 * n_lat * n_lon * (n_wind * (2 + sum(k in addr for k in ("vo", "div", "ws"))) +
                                   n_cols * (C * (1 + sum(k in addr for k in ("col_u", "col_v"))) +
                                             sum(k in addr for k in ("tcwv", "ivtu", "ivtv", "ivt"))))
    _launch(dev, "diagnostics", moved, "aurora_hip_diagnostics", at.get("u"), at.get("v"), at.get("vo"), at.get("div"), at.get("ws"), n_wind,
            _ptr(row_table), float(L), 1 if wrap else 0, at.get("q"), at.get("col_u"), at.get("col_v"), at.get("tcwv"), at.get("ivtu"),
            at.get("ivtv"), at.get("ivt"), n_cols, C, _ptr(level_w), n_lat, n_lon)


# ---- model handle (one forecast step behind the C ABI) ------------------------------------------------------
_PD = ctypes.POINTER(ctypes.c_double)
_PF = ctypes.POINTER(ctypes.c_float)
_PS = ctypes.POINTER(ctypes.c_char_p)


class HipTuning(ctypes.Structure):   # aurora_hip_config.tuning: 0 = the library's default
    _fields_ = [("fuse_ln", c_int32), ("band_split_attention", c_int32), ("qkv_planes", c_int32), ("split_k", c_int32),
                ("perceiver_reassoc", c_int32), ("score_weights", c_int32), ("compose_front", c_int32),
                ("reserved", c_int32 * 1)]


def tuning_from_env() -> HipTuning:
    """The AURORA_* switches of INTEGRATION.md, read HERE (once per handle creation) and handed to the library as fields of
    the configuration: the library itself never reads the environment."""
    t = HipTuning()

    def value(var: str, allowed: tuple[int, ...]):
        raw = os.environ.get(var)
        if raw is None:
            return None
        try:
            v = int(raw.strip())
        except ValueError:
            v = None
        if v not in allowed:   # (a typo must not become the library's default: an A/B run would compare a path with itself)
            raise ValueError(f"{var}={raw!r}: expected one of {', '.join(map(str, allowed))}")
        return v

    v = value("AURORA_FUSE_LN", (0, 1, 2))
    if v is not None:
        t.fuse_ln = v + 1            # 0 / 1 / 2 -> never / fill rule / always
    for field, var in (("band_split_attention", "AURORA_BAND_SPLIT_ATTENTION"), ("qkv_planes", "AURORA_QKV_PLANES"),
                       ("split_k", "AURORA_SPLIT_K"), ("perceiver_reassoc", "AURORA_PERCEIVER_REASSOC"),
                       ("score_weights", "AURORA_SCORE_WEIGHTS"), ("compose_front", "AURORA_COMPOSE_FRONT")):
        v = value(var, (0, 1))
        if v is not None:
            setattr(t, field, 2 if v else 1)
    return t


class HipConfig(ctypes.Structure):   # aurora_hip_config, field for field
    _fields_ = [("embed_dim", c_int32), ("patch_size", c_int32), ("latent_levels", c_int32), ("num_heads", c_int32),
                ("n_stages", c_int32), ("encoder_depths", c_int32 * 4), ("encoder_heads", c_int32 * 4),
                ("decoder_depths", c_int32 * 4), ("decoder_heads", c_int32 * 4), ("window", c_int32 * 3),
                ("enc_depth", c_int32), ("dec_depth", c_int32), ("perceiver_ln_eps", c_float),
                ("max_history", c_int32), ("timestep_hours", ctypes.c_double), ("stabilise_level_agg", c_int32),
                ("use_lora", c_int32), ("lora_steps", c_int32), ("lora_mode", c_int32), ("autocast", c_int32),
                ("n_surf", c_int32), ("n_static", c_int32), ("n_atmos", c_int32),
                ("surf_vars", _PS), ("static_vars", _PS), ("atmos_vars", _PS),
                # variant keywords
                ("variant", c_int32), ("n_level_condition", c_int32), ("level_condition", _PD),
                ("dynamic_vars", c_int32), ("atmos_static_vars", c_int32), ("clamp_at_first_step", c_int32),
                ("simulate_indexing_bug", c_int32),
                ("n_separate_perceiver", c_int32), ("separate_perceiver", _PS),
                ("n_modulation_heads", c_int32), ("modulation_heads", _PS),
                ("difference_history", ctypes.POINTER(c_int32)),
                ("n_positive_surf", c_int32), ("positive_surf_vars", _PS),
                ("n_positive_atmos", c_int32), ("positive_atmos_vars", _PS),
                ("n_surf_inputs", c_int32), ("surf_inputs", _PS),
                ("n_density", c_int32), ("density_channel_surf_vars", _PS),
                ("n_angle", c_int32), ("angle_surf_vars", _PS), ("tuning", HipTuning)]


class HipHaloMsg(ctypes.Structure):   # aurora_hip_halo_msg
    _fields_ = [("peer", c_int32), ("reserved", c_int32), ("offset", c_int64), ("bytes", c_int64)]


HALO_POST_FN = ctypes.CFUNCTYPE(c_int, c_void_p, ctypes.POINTER(HipHaloMsg), c_int32, ctypes.POINTER(HipHaloMsg), c_int32,
                                c_void_p)
HALO_WAIT_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p)


class HipBand(ctypes.Structure):      # aurora_hip_band
    _fields_ = [("rank", c_int32), ("world", c_int32), ("post", HALO_POST_FN), ("wait", HALO_WAIT_FN), ("user", c_void_p)]


class HipGrid(ctypes.Structure):
    _fields_ = [("n_lat", c_int32), ("n_lon", c_int32), ("lat", _PD), ("lon", _PD), ("n_levels", c_int32),
                ("levels", _PD), ("levels_float32", c_int32), ("surf_loc", _PD), ("surf_scale", _PD),
                ("static_loc", _PD), ("static_scale", _PD), ("atmos_loc", _PD), ("atmos_scale", _PD),
                ("pos_encoding", _PF), ("scale_encoding", _PF)]


class HipStepIO(ctypes.Structure):
    _fields_ = [("B", c_int32), ("T", c_int32), ("surf", ctypes.POINTER(c_void_p)), ("surf_strides", c_int64 * 4),
                ("stat", ctypes.POINTER(c_void_p)), ("static_strides", c_int64 * 2),
                ("atmos", ctypes.POINTER(c_void_p)), ("atmos_strides", c_int64 * 5),
                ("out_surf", ctypes.POINTER(c_void_p)), ("out_atmos", ctypes.POINTER(c_void_p)),
                ("rollout_step", c_int32)]


class HipProfileEntry(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_char_p), ("launches", c_int64), ("ms", ctypes.c_double), ("work", ctypes.c_double)]


class HipPlanInfo(ctypes.Structure):
    _fields_ = [("n_windows", c_int32), ("win_tokens", c_int32), ("n_own", c_int32), ("n_halo", c_int32),
                ("n_interior", c_int32), ("recv_offset", c_int32 * 2), ("recv_count", c_int32 * 2),
                ("send_count", c_int32 * 2), ("has_groups", c_int32)]


PROFILE_KINDS = ("linear_bf16", "linear_f32", "window_attention_bf16", "layernorm", "merge_ln", "split_ln", "patchify",
                 "perceiver_attention", "assemble_tokens", "unpatchify", "copy2d", "absmax", "linear_layernorm_bf16",
                 "gather_rows", "perceiver_out")

_SIGNATURES.update({
    "aurora_hip_profile_begin": (c_int, [c_void_p, ctypes.c_uint32]),
    "aurora_hip_profile_end": (c_int, [c_void_p, ctypes.POINTER(HipProfileEntry), c_int, ctypes.POINTER(c_int)]),
    "aurora_hip_profile_end_list": (c_int, [c_void_p, ctypes.POINTER(HipProfileEntry), c_int, ctypes.POINTER(c_int)]),
    "aurora_hip_create": (c_int, [ctypes.POINTER(HipConfig), ctypes.POINTER(c_void_p)]),
    "aurora_hip_destroy": (None, [c_void_p]),
    "aurora_hip_pack_weights": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(c_int64), c_int, c_int, c_int]),
    "aurora_hip_finalize": (c_int, [c_void_p, c_void_p]),
    "aurora_hip_save_packed": (c_int, [c_void_p, ctypes.c_char_p, c_void_p]),
    "aurora_hip_load_packed": (c_int, [c_void_p, ctypes.c_char_p]),
    "aurora_hip_precompute": (c_int, [c_void_p, ctypes.POINTER(HipGrid), c_void_p]),
    "aurora_hip_set_time": (c_int, [c_void_p, _PD, c_int, c_void_p]),
    "aurora_hip_step": (c_int, [c_void_p, ctypes.POINTER(HipStepIO), c_void_p]),
    "aurora_hip_workspace_bytes": (c_int64, [c_void_p]),
    "aurora_hip_guard_words": (c_int, [c_void_p, ctypes.POINTER(c_float), c_void_p]),
    "aurora_hip_guard_limits": (c_int, [c_void_p, ctypes.POINTER(c_float)]),
    "aurora_hip_abi_sizes": (c_int, [ctypes.POINTER(c_int32), c_int]),
    "aurora_hip_generation": (c_int64, [c_void_p]),
    "aurora_hip_compose_weight": (c_int, [_PF, c_int, c_int, _PF, c_int, c_int, _PF]),
    "aurora_hip_compose_bias": (c_int, [_PF, c_int, c_int, _PF, c_int, _PF]),
    "aurora_hip_compose_front_rule": (c_int, [c_int, c_int, ctypes.POINTER(c_int32), c_int]),
    "aurora_hip_composed_value_bound": (c_int, [c_float, c_float, c_float, c_float, c_float, _PF]),
    "aurora_hip_front_composed": (c_int, [c_void_p]),
    "aurora_hip_output_vars": (c_int, [c_void_p, _PS, c_int]),
    "aurora_hip_set_time_ex": (c_int, [c_void_p, _PD, ctypes.POINTER(c_int32), c_int, c_void_p]),
    "aurora_hip_set_band": (c_int, [c_void_p, ctypes.POINTER(HipBand)]),
    "aurora_hip_band_rows": (c_int, [c_void_p, ctypes.POINTER(c_int32), ctypes.POINTER(c_int32)]),
    "aurora_hip_band_staging_bytes": (c_int64, [c_void_p]),
    "aurora_hip_set_band_staging": (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    "aurora_hip_pos_scale_encoding": (c_int, [_PD, _PD, c_int, c_int, c_int, c_int, _PF, _PF]),
    "aurora_hip_band_partition": (c_int, [c_int, ctypes.POINTER(c_int32), ctypes.POINTER(c_int32), c_int, c_int, c_int,
                                          ctypes.POINTER(c_int32), ctypes.POINTER(c_int32)]),
    "aurora_hip_band_plan": (c_int, [ctypes.POINTER(c_int32), ctypes.POINTER(c_int32), c_int, c_int, c_int,
                                     ctypes.POINTER(c_int32), ctypes.POINTER(HipPlanInfo), c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
})
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
