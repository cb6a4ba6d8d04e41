"""ctypes binding of libsinddm_hip.so (the C ABI declared in include/sinddm_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, an
exception is raised.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsinddm_hip.so")

# every symbol include/sinddm_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = (
    "sinddm_abi_version", "sinddm_param_count", "sinddm_param_tensors", "sinddm_param_offset",
    "sinddm_packed_count", "sinddm_workspace_bytes", "sinddm_pack_weights", "sinddm_net_forward",
    "sinddm_q_sample", "sinddm_reverse_step", "sinddm_reverse_step_edit", "sinddm_upsample_bilinear", "sinddm_prof_begin", "sinddm_prof_end", "sinddm_prof_end2", "sinddm_prof_end3", "sinddm_debug_wgrad_map", "sinddm_debug_conv_path",
    "sinddm_debug_block_train", "sinddm_debug_infer_path", "sinddm_debug_train_path",
    "sinddm_train_workspace_bytes", "sinddm_packed_bwd_count", "sinddm_pack_weights_bwd",
    "sinddm_net_forward_train", "sinddm_net_backward", "sinddm_l1_loss_fwd_bwd", "sinddm_adam_ema_step",
    "sinddm_cond_embed", "sinddm_cond_stride", "sinddm_sample_chain", "sinddm_sample_chain2", "sinddm_sample_chain_ex",
    "sinddm_normal_fill", "sinddm_wrap_halo", "sinddm_upsample_bilinear_wrap", "sinddm_sample_chain_tile",
    "sinddm_sample_chain_keep", "sinddm_reverse_step_keep", "sinddm_normal_fill_samples", "sinddm_sample_chain_seeds",
    "sinddm_debug_head_path", "sinddm_debug_head_offsets", "sinddm_debug_head", "sinddm_debug_routes",
    "sinddm_debug_forward_plan",
    "sinddm_debug_wgrad_routes", "sinddm_debug_wgrad_plan", "sinddm_debug_wgrad", "sinddm_debug_wgrad_scratch_bytes",
    "sinddm_sample_chain_resample", "sinddm_reverse_step_jump",
    "sinddm_sample_chain_layout", "sinddm_layout_delta", "sinddm_reverse_step_layout",
    "sinddm_sample_chain_batch",
    "sinddm_sample_chain_solver", "sinddm_reverse_step_ms",
    "sinddm_q_sample_wrap", "sinddm_l1_loss_crop_fwd_bwd",
    "sinddm_sample_chain_mix", "sinddm_normal_fill_mix",
    "sinddm_l1_loss_weighted_fwd_bwd",
    "sinddm_debug_conv_wh", "sinddm_debug_conv_wh_scratch_bytes", "sinddm_debug_conv_wr_proj",
    "sinddm_debug_first_conv",
    "sinddm_patch_nnf_workspace_bytes", "sinddm_patch_nnf",
    "sinddm_q_sample_crop", "sinddm_l1_loss_rect_fwd_bwd",
    "sinddm_sample_chain_gate", "sinddm_reverse_step_keep_gate",
    "sinddm_patch_nnf_scaled_workspace_bytes", "sinddm_patch_nnf_scaled", "sinddm_patch_vote",
    "sinddm_score_workspace_bytes", "sinddm_score_chain",
    "sinddm_normal_fill_window",
    "sinddm_patch_nnf_local",
)


ABI_VERSION = 3               # SINDDM_ABI_VERSION of include/sinddm_hip.h this binding was written against
DIM_FP32_CONVS = 0x10000     # SINDDM_DIM_FP32_CONVS of include/sinddm_hip.h: option bit of every `dim` argument
DIM_HEAD_XIN = 0x20000       # SINDDM_DIM_HEAD_XIN: the collapsed head reads block 4's input, not the conv epilogue's 3-plane projection
JUMP_STREAM = 1 << 31        # SINDDM_JUMP_STREAM of include/sinddm_hip.h: a jump's z2 draw is the step's stream id plus this
MIX_MAX = 4                  # SINDDM_MIX_MAX of include/sinddm_hip.h: seeds per blended sample
SCORE_MAX_EVALS = 1024       # evaluations per sinddm_score_chain call (CHAIN_COND_ROWS of csrc/fwd_plan.h)
TILE_HALO = 16               # SINDDM_TILE_HALO of include/sinddm_hip.h: the network's receptive radius = halo of a wrapped axis


class StepCoefs(C.Structure):
    """Mirror of `sinddm_step_coefs` (include/sinddm_hip.h)."""
    _fields_ = [("mode", C.c_int), ("clip", C.c_int),
                ("sqrt_recip_ac_t", C.c_float), ("sqrt_recipm1_ac_t", C.c_float),
                ("coef1_t", C.c_float), ("coef2_t", C.c_float),
                ("gamma_t", C.c_float), ("gamma_tm1", C.c_float),
                ("sqrt_ac_tm1", C.c_float), ("sqrt_ac_t", C.c_float), ("sqrt_1m_ac_t", C.c_float),
                ("sqrt_1m_ac_tm1_mvar", C.c_float), ("sigma", C.c_float)]


class ChainOpts(C.Structure):
    """Mirror of `sinddm_chain_opts` (include/sinddm_hip.h): device pointers or None."""
    _fields_ = [("edit_w", C.c_void_p), ("edit_c", C.c_void_p), ("noise", C.c_void_p)]


class KeepOpts(C.Structure):
    """Mirror of `sinddm_keep_opts` (include/sinddm_hip.h): `mask` / `x0` device pointers, `ab` a HOST array of
    (keep_a, keep_b) per step of the call."""
    _fields_ = [("mask", C.c_void_p), ("x0", C.c_void_p), ("ab", C.POINTER(C.c_float))]


class JumpCoefs(C.Structure):
    """Mirror of `sinddm_jump_coefs` (include/sinddm_hip.h): the jump that follows a step, or on = 0."""
    _fields_ = [("on", C.c_int), ("r", C.c_float), ("s", C.c_float), ("d", C.c_float)]


class ResampleOpts(C.Structure):
    """Mirror of `sinddm_resample_opts` (include/sinddm_hip.h): `jumps` a HOST array of one entry per step, `noise` a device
    pointer (the z2 draws of the call's jumps, one slot per jump) or None."""
    _fields_ = [("jumps", C.POINTER(JumpCoefs)), ("noise", C.c_void_p)]


class LayoutOpts(C.Structure):
    """Mirror of `sinddm_layout_opts` (include/sinddm_hip.h): `layout` / `delta` device pointers, `down` the block size N, `g`
    a HOST array of one strength per step of the call."""
    _fields_ = [("layout", C.c_void_p), ("down", C.c_int), ("g", C.POINTER(C.c_float)), ("delta", C.c_void_p)]


class BatchOpts(C.Structure):
    """Mirror of `sinddm_batch_opts` (include/sinddm_hip.h): which map families hold one slice per sample, and the device
    pointer of the per-sample layout gains or None."""
    _fields_ = [("edit_per_sample", C.c_int), ("keep_mask_per_sample", C.c_int), ("keep_x0_per_sample", C.c_int),
                ("layout_per_sample", C.c_int), ("layout_gain", C.c_void_p)]


class SolverOpts(C.Structure):
    """Mirror of `sinddm_solver_opts` (include/sinddm_hip.h): `q` a HOST array of one extrapolation factor per step of the
    call (0: a first-order step), `hist` the device buffer that carries the previous step's clean estimate."""
    _fields_ = [("q", C.POINTER(C.c_float)), ("hist", C.c_void_p)]


class MixOpts(C.Structure):
    """Mirror of `sinddm_mix_opts` (include/sinddm_hip.h): `keys` (uint64) / `weights` (float32) device tables of K entries
    per sample, or None."""
    _fields_ = [("keys", C.c_void_p), ("weights", C.c_void_p), ("K", C.c_int)]


class GateOpts(C.Structure):
    """Mirror of `sinddm_gate_opts` (include/sinddm_hip.h): `thr` a HOST array of one threshold in (0, 1] per step of the
    call; the keep mask is then a hold level and a step keeps the pixels whose level is >= its threshold."""
    _fields_ = [("thr", C.POINTER(C.c_float))]


class ScoreOpts(C.Structure):
    """Mirror of `sinddm_score_opts` (include/sinddm_hip.h): `weight` an (H,W) float32 device plane or None (= 1),
    `sample_seeds` a device table of one uint64 seed per sample or None."""
    _fields_ = [("weight", C.c_void_p), ("sample_seeds", C.c_void_p)]


class SinddmError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load (once) and type the library.  Raises if it was not built -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SinddmError(
            f"{LIB_PATH} is missing: build it with `python -m sinddm_amd.build` (hipcc, gfx950). "
            "sinddm_amd has no CPU / PyTorch fallback for the hot path.")
    from . import build as _build
    try:
        _build.verify()                      # a binary built from other sources than the ones beside it is refused
    except RuntimeError as e:
        raise SinddmError(str(e)) from None
    lib = C.CDLL(LIB_PATH)
    p, i, i64, f, sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
    # what every sinddm_sample_chain* entry starts with: params .. stream, aux_stream, result_in_alt
    chain = [p, p, p, p, p, p, C.POINTER(StepCoefs), C.POINTER(C.c_int), i, f, C.c_uint64, C.c_uint64, i, i, i, i, p, sz, p, p,
             C.POINTER(C.c_int)]
    sig = {
        "sinddm_abi_version": (i, []),
        "sinddm_param_count": (i64, [i]),
        "sinddm_param_tensors": (i, [i]),
        "sinddm_param_offset": (i64, [i, i]),
        "sinddm_packed_count": (i64, [i]),
        "sinddm_workspace_bytes": (sz, [i, i, i, i]),
        "sinddm_pack_weights": (i, [p, p, i, p]),
        "sinddm_net_forward": (i, [p, p, p, p, i, f, p, i, i, i, i, p, sz, p]),
        "sinddm_cond_embed": (i, [p, p, i, f, i, i, p, p, p, p]),
        "sinddm_cond_stride": (i, [i]),
        "sinddm_q_sample": (i, [p, p, p, p, p, p, p, p, i, i, i64, p]),
        "sinddm_q_sample_wrap": (i, [p, p, p, p, p, p, p, p, i, i, i, i, i, i, i, p]),
        "sinddm_reverse_step": (i, [p, p, p, p, p, C.POINTER(StepCoefs), i64, p]),
        "sinddm_reverse_step_edit": (i, [p, p, p, p, p, C.POINTER(StepCoefs), p, p, i, i, i, p]),
        "sinddm_sample_chain": (i, chain[:-2] + [C.POINTER(C.c_int)]),                      # (no aux_stream)
        "sinddm_sample_chain2": (i, chain),
        "sinddm_sample_chain_ex": (i, chain + [C.POINTER(ChainOpts)]),
        "sinddm_sample_chain_tile": (i, chain + [C.POINTER(ChainOpts), i, i]),
        "sinddm_sample_chain_keep": (i, chain + [C.POINTER(ChainOpts), i, i, C.POINTER(KeepOpts)]),
        "sinddm_sample_chain_seeds": (i, chain + [C.POINTER(ChainOpts), i, i, C.POINTER(KeepOpts), p]),
        "sinddm_sample_chain_resample": (i, chain + [C.POINTER(ChainOpts), i, i, C.POINTER(KeepOpts), p,
                                                     C.POINTER(ResampleOpts)]),
        "sinddm_sample_chain_layout": (i, chain + [C.POINTER(ChainOpts), i, i, C.POINTER(KeepOpts), p,
                                                   C.POINTER(ResampleOpts), C.POINTER(LayoutOpts)]),
        "sinddm_sample_chain_batch": (i, chain + [C.POINTER(ChainOpts), i, i, C.POINTER(KeepOpts), p,
                                                  C.POINTER(ResampleOpts), C.POINTER(LayoutOpts), C.POINTER(BatchOpts)]),
        "sinddm_sample_chain_solver": (i, chain + [C.POINTER(ChainOpts), i, i, C.POINTER(KeepOpts), p,
                                                   C.POINTER(ResampleOpts), C.POINTER(LayoutOpts), C.POINTER(BatchOpts),
                                                   C.POINTER(SolverOpts)]),
        "sinddm_sample_chain_mix": (i, chain + [C.POINTER(ChainOpts), i, i, C.POINTER(KeepOpts), p,
                                                C.POINTER(ResampleOpts), C.POINTER(LayoutOpts), C.POINTER(BatchOpts),
                                                C.POINTER(SolverOpts), C.POINTER(MixOpts)]),
        "sinddm_sample_chain_gate": (i, chain + [C.POINTER(ChainOpts), i, i, C.POINTER(KeepOpts), p,
                                                 C.POINTER(ResampleOpts), C.POINTER(LayoutOpts), C.POINTER(BatchOpts),
                                                 C.POINTER(SolverOpts), C.POINTER(MixOpts), C.POINTER(GateOpts)]),
        "sinddm_normal_fill_mix": (i, [p, i, i64, p, p, i, C.c_uint64, p]),
        "sinddm_normal_fill_window": (i, [p, i, p, i, i, i, p, i, i, p, p, i, p]),
        "sinddm_reverse_step_ms": (i, [p, p, p, p, p, C.POINTER(StepCoefs), f, p, p, p, p, p, f, f, i, i, i, p]),
        "sinddm_layout_delta": (i, [p, p, p, p, p, C.POINTER(StepCoefs), p, p, i, i, i, i, i, i, p]),
        "sinddm_reverse_step_layout": (i, [p, p, p, p, p, C.POINTER(StepCoefs), p, f, i, p, p, p, p, f, f, i, i, i, i, i, i, i,
                                           p]),
        "sinddm_reverse_step_jump": (i, [p, p, p, p, p, p, C.POINTER(StepCoefs), C.POINTER(JumpCoefs), p, p, p, p, f, f, i, i, i,
                                         p]),
        "sinddm_normal_fill_samples": (i, [p, i, i64, p, C.c_uint64, p]),
        "sinddm_reverse_step_keep": (i, [p, p, p, p, p, C.POINTER(StepCoefs), p, p, p, p, f, f, i, i, i, p]),
        "sinddm_reverse_step_keep_gate": (i, [p, p, p, p, p, C.POINTER(StepCoefs), p, p, p, p, f, f, i, i, i, p, f]),
        "sinddm_wrap_halo": (i, [p, p, i, i, i, i, i, p]),
        "sinddm_upsample_bilinear_wrap": (i, [p, p, i, i, i, i, i, i, i, p]),
        "sinddm_normal_fill": (i, [p, i64, C.c_uint64, C.c_uint64, p]),
        "sinddm_upsample_bilinear": (i, [p, p, i, i, i, i, i, p]),
        "sinddm_prof_begin": (i, []),
        "sinddm_prof_end": (i, [C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
        "sinddm_prof_end2": (i, [C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double)]),
        "sinddm_prof_end3": (i, [i, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), i]),
        "sinddm_debug_wgrad_map": (i, [i, i, i64, i, C.POINTER(C.c_uint32), i, C.POINTER(C.c_int32), i]),
        "sinddm_debug_conv_path": (i, [i, i, i, i]),
        "sinddm_debug_infer_path": (i, [i, i, i, i]),
        "sinddm_debug_train_path": (i, [i, i, i, i]),
        "sinddm_debug_head_path": (i, [i, i, i, i]),
        "sinddm_debug_routes": (i, [i, i, i, i, i, C.POINTER(C.c_int)]),
        "sinddm_debug_wgrad_routes": (i, [i, i, i, i, i, C.POINTER(C.c_int), i]),
        "sinddm_debug_wgrad_plan": (i, [i, i, i, i, i, i, i, i, i, C.POINTER(C.c_int)]),
        "sinddm_debug_wgrad": (i, [i, i, i, i, i, i, i, i, i, p, p, p, p, p, sz, C.POINTER(C.c_int), p]),
        "sinddm_debug_wgrad_scratch_bytes": (sz, [i, i, i, i]),
        "sinddm_debug_conv_wh": (i, [i, i, i, i, i, i, i, i, i, p, p, p, p, p, p, p, p, p, sz, p]),
        "sinddm_debug_conv_wh_scratch_bytes": (sz, [i, i, i]),
        "sinddm_debug_conv_wr_proj": (i, [i, i, i, i, i, i, i, p, p, p, p, p, p, p, p, sz, p]),
        "sinddm_debug_first_conv": (i, [i, i, i, i, i, i, i, p, p, p, p, p, p]),
        "sinddm_debug_head_offsets": (i, [i, C.POINTER(C.c_int64)]),
        "sinddm_debug_forward_plan": (i, [i, i, i, i, i, i, C.POINTER(C.c_int64), i]),
        "sinddm_debug_head": (i, [p, p, p, p, i, i, i, i, i, p]),
        "sinddm_debug_block_train": (i, [p, p, p, i, i, p, p, p, p, p, p, p, i, i, i, p, sz, p]),
        "sinddm_train_workspace_bytes": (sz, [i, i, i, i]),
        "sinddm_packed_bwd_count": (i64, [i]),
        "sinddm_pack_weights_bwd": (i, [p, p, i, p]),
        "sinddm_net_forward_train": (i, [p, p, p, p, i, f, p, i, i, i, i, p, sz, p]),
        "sinddm_net_backward": (i, [p, p, p, p, p, p, p, i, i, i, i, p, sz, p]),
        "sinddm_l1_loss_fwd_bwd": (i, [p, p, p, p, i64, f, p]),
        "sinddm_l1_loss_crop_fwd_bwd": (i, [p, p, p, p, i, i, i, i, i, f, p]),
        "sinddm_l1_loss_weighted_fwd_bwd": (i, [p, p, p, p, p, i, i, i, i, i, i, f, f, p]),
        "sinddm_q_sample_crop": (i, [p, p, p, p, p, p, p, p, i, p, i, i, i, i, i, i, p]),
        "sinddm_l1_loss_rect_fwd_bwd": (i, [p, p, p, p, p, p, p, i, i, i, i, i, i, f, f, p]),
        "sinddm_adam_ema_step": (i, [p, p, p, p, p, f, f, f, f, f, f, f, i, i64, p]),
        "sinddm_patch_nnf_workspace_bytes": (sz, [i, i, i, i, i, i, i, i]),
        "sinddm_patch_nnf": (i, [p, i, p, i, p, p, p, i, i, i, i, i, i, i, i, p, sz, p]),
        "sinddm_patch_nnf_scaled_workspace_bytes": (sz, [i, i, i, i, i, i, i, i]),
        "sinddm_patch_nnf_scaled": (i, [p, i, p, i, p, p, i, p, p, i, i, i, i, i, i, i, i, p, sz, p]),
        "sinddm_patch_vote": (i, [p, p, i, p, p, i, p, i, i, i, i, i, i, i, i, f, p]),
        "sinddm_patch_nnf_local": (i, [p, i, p, i, p, p, i, p, i, p, p, i, i, i, i, i, i, i, i, p]),
        "sinddm_score_workspace_bytes": (sz, [i, i, i, i, i]),
        "sinddm_score_chain": (i, [p, p, p, p, p, p, p, p, C.POINTER(C.c_int), i, f, C.c_uint64, C.c_uint64, p, p, i, i, i, i,
                                   p, sz, p, C.POINTER(ScoreOpts)]),
    }
    for name, (res, args) in sig.items():
        if not hasattr(lib, name):
            continue  # reported by check_symbols(); calling it raises AttributeError loudly
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def missing_symbols():
    lib = load()
    return [s for s in ABI_SYMBOLS if not hasattr(lib, s)]


def check(rc: int, what: str) -> None:
    if rc != 0:
        kind = {-1: "bad argument", -2: "unsupported shape", -3: "workspace too small"}.get(rc, f"hipError {rc}")
        raise SinddmError(f"{what} failed: {kind}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise SinddmError("sinddm_amd kernels need tensors on a ROCm device (no CPU fallback)")
    if not t.is_contiguous():
        raise SinddmError("sinddm_amd kernels need contiguous tensors")
    return t.data_ptr()


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream
