"""SinDDMNet and MultiScaleGaussianDiffusion backed by the gfx950 HIP library.

Same Python surface as the reference (SinDDM/models.py): constructor signatures, method names,
state-dict keys and buffer names are kept so `main.py` / `MultiscaleTrainer` and existing
checkpoints work unchanged, while every per-step tensor op runs in libsinddm_hip.so:

  SinDDMNet.forward          -> sinddm_net_forward        (models.py:134-151)
  q_sample / p_losses mix    -> sinddm_q_sample           (models.py:570-590)
  p_losses' options          -> sinddm_q_sample_wrap, sinddm_l1_loss_crop_fwd_bwd / _weighted_fwd_bwd   (`train_tile`,
                                `train_weights`; no reference line: one plan per step, train_step.TrainStep);
                                sinddm_q_sample_crop, sinddm_l1_loss_rect_fwd_bwd   (`train_crop`: a window per sample)
  p_sample tail              -> sinddm_reverse_step       (models.py:306-352,433-459)
  inter-scale upsample       -> sinddm_upsample_bilinear  (models.py:567)
  known pixels (`keep_maps`) -> sinddm_sample_chain_keep / sinddm_reverse_step_keep   (no reference line: RePaint-style
                                replacement of the known region after every reverse step)
  edit strength (`keep_gated`) -> sinddm_sample_chain_gate / sinddm_reverse_step_keep_gate   (no reference line: the keep
                                gated per pixel by the step's level -- each pixel its own SDEdit start level)
  tileable sampling (`tile`) -> sinddm_sample_chain_tile / sinddm_wrap_halo / sinddm_upsample_bilinear_wrap
                                (no reference line: padding_mode='circular' on its nn.Conv2d's)
  per-sample noise seeds     -> sinddm_sample_chain_seeds / sinddm_normal_fill_samples   (`sample_seeds`; no reference
                                line: the reference never seeds its generator)
  seed blending (`seed_mix`) -> sinddm_sample_chain_mix / sinddm_normal_fill_mix   (no reference line: a sample's draw as
                                a fixed combination of the draws of K seeds -- interpolations and loops between samples)
  windowed keep (`keep_window`) -> sinddm_normal_fill_window   (no reference line: a known-region run evaluated on the
                                window around its free pixels, with the draws of the full run)
  few-step sampling          -> strided step scalars (`step_coefs_to`) through every chain entry; `solver_order = 2`:
                                sinddm_sample_chain_solver / sinddm_reverse_step_ms   (no reference line: the reference
                                evaluates the network at every level)

There is no CPU / eager-PyTorch fallback: tensors must live on a ROCm device and the shared
library must be built, otherwise calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
from contextlib import contextmanager
from functools import partial
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .autograd import l1_loss
from .functions import cosine_beta_schedule, crop_windows, default, exists, extract, noise_like
from .sampler import SAMPLING_OPTIONS, RunPlan, pack_steps, refuse, sampling_defaults
from .synth import net_param_shapes
from .train_step import TrainStep


# --------------------------------------------------------------------------------------------
# EMA (reference models.py:18-31) -- the trainer uses the fused kernel; this stays for API parity
# --------------------------------------------------------------------------------------------
class EMA:
    def __init__(self, beta):
        self.beta = beta

    def update_model_average(self, ma_model, current_model):
        for cur, ma in zip(current_model.parameters(), ma_model.parameters()):
            ma.data = self.update_average(ma.data, cur.data)

    def update_average(self, old, new):
        if old is None:
            return new
        return old * self.beta + (1 - self.beta) * new


class SinusoidalPosEmb(nn.Module):
    """[sin(x f_i) | cos(x f_i)] (models.py:34-46).  Exposed for API parity; SinDDMNet computes the
    embedding inside its conditioning kernel."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        half = self.dim // 2
        k = math.log(10000) / (half - 1)
        f = torch.exp(torch.arange(half, device=x.device) * -k)
        arg = x[:, None] * f[None, :]
        return torch.cat((arg.sin(), arg.cos()), dim=-1)


# --------------------------------------------------------------------------------------------
# scratch memory shared by all nets on a device (PyTorch = allocator only)
# --------------------------------------------------------------------------------------------
_WS: Dict[Tuple[str, int], torch.Tensor] = {}


def _workspace(device: torch.device, nbytes: int, tag: str = "fwd") -> torch.Tensor:
    device = torch.device(device)
    key = (tag, device.index if device.index is not None else torch.cuda.current_device())
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = None
        _WS.pop(key, None)
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


# Byte budget of one noise buffer of a `chain_noise` run (MultiScaleGaussianDiffusion._run_steps): the steps of a run are
# cut into pieces whose recorded draws fit.  1 GiB is 6 steps of C3's finest scale at batch 64 (161 MB per step) and the
# whole 521-step run of C2's 67x90 scale at batch 16 (1.2 MB per step).
CHAIN_NOISE_BYTES = 1 << 30

# ---- per-sample noise seeds (include/sinddm_hip.h "the noise contract") -------------------------------------
SEED_LIMIT = 1 << 63          # a sample seed is a Python int in [0, 2^63): 8 bytes on the device
_STREAM_KINDS = {"init": 0, "renoise": 1, "step": 2, "jump": _lib.JUMP_STREAM + 2}


def noise_stream_id(s: int, kind: str, i: int = 0) -> int:
    """Stream id of one draw of a seeded sample: (s << 32) | k with k = 0 the initial draw of p_sample_loop at scale s,
    k = 1 the re-noise draw of p_sample_via_scale_loop, k = 2 + i the reverse step at position i of the scale's run (counted
    from the run's first step), k = 2^31 + 2 + i the second draw (z2) of the resampling jump that follows the step at position
    i of the EXPANDED walk (i < 2^31 - 2, which a run with jumps also keeps its steps below: the library adds
    SINDDM_JUMP_STREAM to the step's id).  The ONE owner of this layout: the fused route hands noise_stream_id(s, "step", 0)
    to the library as stream_id0, the step-by-step route asks for every position."""
    k = _STREAM_KINDS[kind]
    s, i = int(s), int(i)
    if kind not in ("step", "jump") and i != 0:
        raise ValueError(f"the {kind!r} draw of a scale has no position")
    if not (0 <= s < (1 << 31)) or not (0 <= i < ((1 << 31) if kind == "jump" else (1 << 32)) - 2):
        raise ValueError(f"noise_stream_id: scale {s} / position {i} out of range")
    return (s << 32) | (k + i)


_M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    """One output of splitmix64 (Steele, Lea, Flood 2014) for the state x: a bijection of the 64-bit integers."""
    z = (int(x) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _check_seed_row(row, what: str = "sample_seeds"):
    out = []
    for v in row:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: a seed must be an int, got {v!r}")
        v = int(v)
        if not 0 <= v < SEED_LIMIT:
            raise ValueError(f"{what}: seed {v} is outside [0, 2^63)")
        out.append(v)
    return out


def vary_seeds(seeds, from_scale: int, n_scales: int):
    """The 2-D [n_scales][B] form of `sample_seeds` for SinGAN-style variations: scales below `from_scale` keep `seeds`,
    every scale from `from_scale` on uses derived seeds -- same coarse structure, fresh fine detail.  Sample b's derived seed
    is splitmix64(seeds[b] ^ splitmix64(b + 1)) >> 1 (63 bits); should it equal the derived seed of an earlier sample of the
    row, splitmix64 is applied again until it does not.  So the result is a pure function of (seeds, from_scale, n_scales),
    and derived seeds are distinct for distinct b even when the given seeds are equal."""
    seeds = _check_seed_row(seeds, "vary_seeds")
    from_scale, n_scales = int(from_scale), int(n_scales)
    if not 0 <= from_scale <= n_scales:
        raise ValueError(f"vary_seeds: from_scale {from_scale} is outside [0, {n_scales}]")
    derived, used = [], set()
    for b, v in enumerate(seeds):
        z = _splitmix64(v ^ _splitmix64(b + 1))
        while (z >> 1) in used:
            z = _splitmix64(z)
        used.add(z >> 1)
        derived.append(z >> 1)
    return [list(seeds) if s < from_scale else list(derived) for s in range(n_scales)]


# ---- seed blending (include/sinddm_hip.h "seed blending") ---------------------------------------------------
# A mix is a pair (keys, weights) of [B][K] nested sequences: sample b's every N(0,1) draw is sum_k weights[b][k] * (the draw
# of seed keys[b][k]), which is N(0,1) again when the row's squared weights add up to 1.  The helpers below are host code.
MIX_TOL = 1e-5                # |sum_k w^2 - 1| a row of `seed_mix` may have


def _check_mix(keys, weights, what: str = "seed_mix"):
    """The validated ([B][K] ints, [B][K] floats) of one mix table."""
    keys = [list(r.tolist() if isinstance(r, (np.ndarray, torch.Tensor)) else r) for r in keys]
    weights = [list(r.tolist() if isinstance(r, (np.ndarray, torch.Tensor)) else r) for r in weights]
    if len(keys) != len(weights) or not keys:
        raise ValueError(f"{what}: {len(keys)} rows of seeds for {len(weights)} rows of weights")
    K = len(keys[0])
    if not 1 <= K <= _lib.MIX_MAX:
        raise ValueError(f"{what}: {K} seeds per sample, 1 .. {_lib.MIX_MAX} can be blended")
    out_k, out_w = [], []
    for kr, wr in zip(keys, weights):
        if len(kr) != K or len(wr) != K:
            raise ValueError(f"{what}: every row holds the same number of seeds and weights ({K})")
        out_k.append(_check_seed_row(kr, what))
        wr = [float(v) for v in wr]
        if not all(math.isfinite(v) for v in wr):
            raise ValueError(f"{what}: a weight is not finite: {wr}")
        if abs(sum(v * v for v in wr) - 1.0) > MIX_TOL:
            raise ValueError(f"{what}: the squared weights of a row must add up to 1 (unit variance), got {wr}")
        out_w.append(wr)
    return out_k, out_w


def interp_seeds(a: int, b: int, frames: int):
    """The mix that walks from sample `a` (frame 0) to sample `b` (the last frame) on a quarter circle: K = 2, weights
    (cos th_i, sin th_i), th_i = i / (frames - 1) * pi / 2; the end rows are exactly (1, 0) and (0, 1)."""
    a, b = _check_seed_row([a, b], "interp_seeds")
    frames = int(frames)
    if frames < 2:
        raise ValueError(f"interp_seeds: {frames} frames, at least 2 are needed")
    w = []
    for i in range(frames):
        th = i / (frames - 1) * (math.pi / 2)
        w.append([1.0, 0.0] if i == 0 else [0.0, 1.0] if i == frames - 1 else [math.cos(th), math.sin(th)])
    return [[a, b] for _ in range(frames)], w


def loop_seeds(base: int, a: int, b: int, frames: int, radius: float = 0.5):
    """The mix of a closed loop around sample `base`: K = 3, weights (sqrt(1 - r^2), r cos ph_i, r sin ph_i),
    ph_i = 2 pi i / frames -- frame `frames` would be frame 0 again."""
    base, a, b = _check_seed_row([base, a, b], "loop_seeds")
    frames, r = int(frames), float(radius)
    if frames < 1:
        raise ValueError(f"loop_seeds: {frames} frames")
    if not 0.0 <= r <= 1.0:
        raise ValueError(f"loop_seeds: radius {radius} is outside [0, 1]")
    c = math.sqrt(1.0 - r * r)
    return ([[base, a, b] for _ in range(frames)],
            [[c, r * math.cos(2 * math.pi * i / frames), r * math.sin(2 * math.pi * i / frames)] for i in range(frames)])


def mix_from_scale(mix, from_scale: int, n_scales: int):
    """The [n_scales][B][K] form of a mix in which the scales below `from_scale` use each row's FIRST seed alone (weight 1,
    the others 0) and the scales from `from_scale` on the mix itself: a shared coarse layout -- where the rows share their
    first seed -- with detail that moves."""
    keys, w = _check_mix(*mix, what="mix_from_scale")
    from_scale, n_scales = int(from_scale), int(n_scales)
    if not 0 <= from_scale <= n_scales:
        raise ValueError(f"mix_from_scale: from_scale {from_scale} is outside [0, {n_scales}]")
    first = [[1.0] + [0.0] * (len(r) - 1) for r in w]
    return ([[list(r) for r in keys] for _ in range(n_scales)],
            [[list(r) for r in (first if s < from_scale else w)] for s in range(n_scales)])


_AUX: Dict[int, "torch.cuda.Stream"] = {}


def _aux_stream(device: torch.device) -> int:
    """A second stream per device for sinddm_sample_chain2 (coarse scales run as two overlapping half-batches)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _AUX.get(idx)
    if st is None:
        st = torch.cuda.Stream(device=idx)
        _AUX[idx] = st
    return st.cuda_stream


class _Leaf(nn.Module):
    """Holds one (weight, bias) pair under the reference's key names."""

    def __init__(self, wshape, fan_in):
        super().__init__()
        w = torch.empty(wshape)
        # torch default init of nn.Conv2d / nn.Linear (kaiming_uniform a=sqrt(5); bias U(+-1/sqrt(fan_in)))
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
        b = torch.empty(wshape[0]).uniform_(-bound, bound)
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(b)


def _container(children: Dict[str, nn.Module]) -> nn.Module:
    m = nn.Module()
    for k, v in children.items():
        m.add_module(k, v)
    return m


class SinDDMNet(nn.Module):
    """4-block fully-convolutional eps-predictor conditioned on (t, s) -- reference
    SinDDM/models.py:85-151 -- executed by hand-written gfx950 kernels.

    All 52 parameter tensors are views into ONE flat fp32 buffer laid out in nn.Module
    registration order (what the C ABI expects); gradients likewise, so the fused Adam/EMA
    kernel walks a single array."""

    # per-call kernel option of the C ABI (include/sinddm_hip.h, SINDDM_DIM_FP32_CONVS): True keeps every 3x3 conv of this net's
    # launches on the fp32 matrix pipe -- A/B measurements and parity tests (set it on an instance, or on the class for every
    # net a test builds); no reference counterpart
    fp32_convs = False
    # ... and SINDDM_DIM_HEAD_XIN: True keeps the collapsed head on block 4's whole input where block 3's second conv would
    # hand it the 3-plane projection from its epilogue (dim = 160 at the finest scales) -- the same uses
    head_xin = False

    def __init__(self, dim, out_dim=None, channels=3, with_time_emb=True, multiscale=False, device=None):
        super().__init__()
        if not with_time_emb or not multiscale:
            # (not a gap against the reference: its forward tests `exists(self.multiscale)` -- true for False as well -- and then
            # dereferences SinEmbTime / SinEmbScale, which only the multiscale=True, with_time_emb=True constructor creates
            # (models.py:99-118,136-141): multiscale=False raises AttributeError at the first forward there, with_time_emb=False a TypeError in the constructor -- checked against the reference)
            raise NotImplementedError("the MI355X build implements the configuration main.py uses: "
                                      "with_time_emb=True, multiscale=True (reference main.py:77-81); the reference's own forward "
                                      "cannot run any other combination (models.py:136-141)")
        if channels != 3 or default(out_dim, channels) != 3:
            raise NotImplementedError("channels=3 / out_dim=3 only (reference main.py:77-81, models.py:129)")
        self.device = device
        self.channels = channels
        self.multiscale = multiscale
        self.dim = int(dim)
        time_dim = 32
        half = int(dim / 2)
        self.SinEmbTime = SinusoidalPosEmb(time_dim)
        self.SinEmbScale = SinusoidalPosEmb(time_dim)
        self.time_mlp = _container({"0": _Leaf((time_dim * 4, time_dim * 2), time_dim * 2),
                                    "2": _Leaf((time_dim, time_dim * 4), time_dim * 4)})
        for name, (cin, cout) in zip(("l1", "l2", "l3", "l4"),
                                     ((channels, half), (half, dim), (dim, dim), (dim, half))):
            kids = {
                "mlp": _container({"1": _Leaf((time_dim, time_dim), time_dim)}),
                "time_reshape": _Leaf((cin, time_dim, 1, 1), time_dim),
                "ds_conv": _Leaf((cin, 1, 5, 5), 25),
                "net": _container({"0": _Leaf((cout, cin, 3, 3), cin * 9), "2": _Leaf((cout, cout, 3, 3), cout * 9)}),
            }
            if cin != cout:
                kids["res_conv"] = _Leaf((cout, cin, 1, 1), cin)
            self.add_module(name, _container(kids))
        self.final_conv = _container({"0": _Leaf((channels, half, 1, 1), half)})

        self._flat: Optional[torch.Tensor] = None
        self._flat_grad: Optional[torch.Tensor] = None
        self._packed: Optional[torch.Tensor] = None
        self._packed_bwd: Optional[torch.Tensor] = None
        self._packed_version = -1
        self._packed_bwd_version = -1
        self._dirty = 0
        expected = net_param_shapes(self.dim, channels)
        got = {k: tuple(v.shape) for k, v in self.named_parameters()}
        assert list(got.items()) == list(expected.items()), "parameter layout drifted from the reference key order"
        self._flatten()

    # ---- flat parameter storage ---------------------------------------------------------
    def _flatten(self):
        params = list(self.parameters())
        dev = params[0].device
        total = sum(p.numel() for p in params)
        flat = torch.empty(total, dtype=torch.float32, device=dev)
        grad = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in params:
                n = p.numel()
                flat[off:off + n].copy_(p.data.reshape(-1).to(torch.float32))
                p.data = flat[off:off + n].view(p.shape)
                p.grad = None
                off += n
        self._flat, self._flat_grad = flat, grad
        self._packed = None
        self._packed_bwd = None
        self._packed_version = self._packed_bwd_version = -1

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._flatten()
        return out

    def bind_grads(self):
        """Point every p.grad at its slice of the flat gradient buffer (idempotent)."""
        off = 0
        for p in self.parameters():
            n = p.numel()
            g = self._flat_grad[off:off + n].view(p.shape)
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g
            off += n

    @property
    def flat_params(self) -> torch.Tensor:
        return self._flat

    @property
    def flat_grads(self) -> torch.Tensor:
        return self._flat_grad

    def _autograd_anchor(self) -> torch.Tensor:
        a = getattr(self, "_anchor", None)
        if a is None or a.device != self._flat.device:
            a = torch.zeros((), device=self._flat.device, requires_grad=True)
            self._anchor = a
        return a

    def mark_dirty(self):
        """Call after the parameters were changed through raw pointers (fused optimizer)."""
        self._dirty += 1

    def _param_version(self) -> int:
        # in-place updates through the nn.Parameter views (load_state_dict, torch optimizers) bump the
        # parameters' own version counters; raw-pointer updates call mark_dirty()
        return sum(p._version for p in self.parameters()) + (self._dirty << 32)

    def __deepcopy__(self, memo):
        # the EMA copy (trainer.py:100 in the reference) must own its own flat buffer
        new = type(self)(dim=self.dim, channels=self.channels, multiscale=True, device=self.device)
        new.to(self._flat.device)
        with torch.no_grad():
            new._flat.copy_(self._flat)
        for p_new, p_old in zip(new.parameters(), self.parameters()):
            p_new.requires_grad_(p_old.requires_grad)
        new.train(self.training)
        memo[id(self)] = new
        return new

    def _check_lib_layout(self):
        lib = _lib.load()
        n = lib.sinddm_param_count(self.dim)
        if n != self._flat.numel():
            raise _lib.SinddmError(f"parameter count mismatch: python {self._flat.numel()} vs library {n}")

    def packed_weights(self) -> torch.Tensor:
        """MFMA-ready weight image; rebuilt on device whenever the parameters changed."""
        lib = _lib.load()
        v = self._param_version()
        if self._packed is None or self._packed_version != v:
            if self._packed is None:
                self._check_lib_layout()
                self._packed = torch.empty(lib.sinddm_packed_count(self.dim), dtype=torch.float32,
                                           device=self._flat.device)
            _lib.check(lib.sinddm_pack_weights(_lib.ptr(self._flat), _lib.ptr(self._packed), self.dim,
                                               _lib.stream_ptr(self._flat.device)), "sinddm_pack_weights")
            self._packed_version = v
        return self._packed

    def packed_weights_bwd(self) -> torch.Tensor:
        lib = _lib.load()
        v = self._param_version()
        if self._packed_bwd is None or self._packed_bwd_version != v:
            if self._packed_bwd is None:
                self._packed_bwd = torch.empty(lib.sinddm_packed_bwd_count(self.dim), dtype=torch.float32,
                                               device=self._flat.device)
            _lib.check(lib.sinddm_pack_weights_bwd(_lib.ptr(self._flat), _lib.ptr(self._packed_bwd), self.dim,
                                                   _lib.stream_ptr(self._flat.device)), "sinddm_pack_weights_bwd")
            self._packed_bwd_version = v
        return self._packed_bwd

    # ---- forward ------------------------------------------------------------------------
    def infer(self, x: torch.Tensor, t_dev: Optional[torch.Tensor], t_host: int, scale: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Inference forward (no saved activations).  `t_dev` (B,) int64 or None -> all samples
        use the host integer `t_host` (the sampler's case, models.py:481,541)."""
        lib = _lib.load()
        if not x.is_cuda:
            raise _lib.SinddmError("SinDDMNet needs a ROCm device tensor: there is no CPU fallback")
        x = x.contiguous()
        if x.dtype != torch.float32:
            raise _lib.SinddmError("fp32 only")
        B, Cc, H, W = x.shape
        assert Cc == self.channels
        if out is None:
            out = torch.empty_like(x)
        packed = self.packed_weights()
        nbytes = lib.sinddm_workspace_bytes(self.dim, B, H, W)
        ws = _workspace(x.device, nbytes)
        if t_dev is not None:
            t_dev = t_dev.to(device=x.device, dtype=torch.int64).contiguous()
        _lib.check(lib.sinddm_net_forward(_lib.ptr(self._flat), _lib.ptr(packed), _lib.ptr(x),
                                          _lib.ptr(t_dev) if t_dev is not None else None, int(t_host),
                                          float(scale), _lib.ptr(out), self.dim_arg, B, H, W, ws.data_ptr(),
                                          ws.numel(), _lib.stream_ptr(x.device)), "sinddm_net_forward")
        return out

    @property
    def dim_arg(self) -> int:
        """The `dim` argument of the launching C-ABI calls: the width + this net's option bits."""
        return self.dim | (_lib.DIM_FP32_CONVS if self.fp32_convs else 0) | (_lib.DIM_HEAD_XIN if self.head_xin else 0)

    def forward(self, x, time, scale=None):
        """eps = net(x, time, scale) -- same call signature as the reference (models.py:134)."""
        s = float(scale) if scale is not None else 0.0
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if needs_grad:
            from .autograd import net_forward_train
            return net_forward_train(self, x, time, s)
        return self.infer(x, time, 0, s)


# --------------------------------------------------------------------------------------------
# diffusion process
# --------------------------------------------------------------------------------------------
class _ChainCall:
    """The buffers and option blocks of one chain run of `MultiScaleGaussianDiffusion._run_steps`: the steps of `plan` (a
    sampler.RunPlan) on `img`, through sinddm_sample_chain_batch -- or the later entry that can express the run's options
    (_solver, _mix, _gate); one that is off goes in as NULL, which is the call without it, launch for launch.  Every tensor and ctypes array the library reads through
    a raw pointer is an attribute here, so it lives as long as the object."""

    def __init__(self, d, plan, img):
        self.lib, self.net, self.s, self.plan = _lib.load(), d.denoise_fn, plan.s, plan
        hy, hx = self.halo = plan.halo
        tiled = self.tiled = bool(hy or hx)
        wrap = (lambda t: d._wrap_pad(t, hy, hx)) if tiled else (lambda t: t)
        self.Hc, self.Wc = int(img.shape[2]), int(img.shape[3])    # the sample's own size; H, W below: the buffers' size
        x = self.x = d._wrap_pad(img, hy, hx) if tiled else img.contiguous().clone()
        self.x_alt, self.eps = torch.empty_like(x), torch.empty_like(x)
        B, _, H, W = x.shape
        xt = plan.xt
        if xt is not None and (xt.shape != img.shape or xt.dtype != x.dtype or xt.device != x.device):
            # (the library takes raw pointers: a mismatching x-tilde would be read out of bounds)
            raise _lib.SinddmError(f"img_prev_upsample {tuple(xt.shape)} {xt.dtype} {xt.device} does not match the "
                                   f"running sample {tuple(img.shape)} {x.dtype} {x.device}")
        self.xt = wrap(xt) if xt is not None else None
        self.packed = self.net.packed_weights()
        self.ws = _workspace(x.device, self.lib.sinddm_workspace_bytes(self.net.dim, B, H, W))
        # the option blocks: the maps (wrapped under a halo) go in here, the per-step host arrays with each call
        self.edit = [wrap(m) for m in plan.roi] if plan.roi is not None else (None, None)
        self.opts = _lib.ChainOpts(_lib.ptr(self.edit[0]), _lib.ptr(self.edit[1]), None)
        self.kopts = self.lopts = self.bopts = self.sopts = self.hist = None
        self.gopts = _lib.GateOpts() if plan.gated else None
        if plan.keep is not None:
            self.keep = [wrap(m) for m in plan.keep]
            self.kopts = _lib.KeepOpts(_lib.ptr(self.keep[0]), _lib.ptr(self.keep[1]), None)
        self.ropts = _lib.ResampleOpts() if plan.jump_to is not None else None
        self.gain = torch.from_numpy(plan.gain.copy()).to(x.device) if plan.gain is not None else None
        if any(plan.per) or self.gain is not None:
            self.bopts = _lib.BatchOpts(*plan.per, _lib.ptr(self.gain))
        if plan.lay is not None:
            N = plan.lay[1]
            self.lay_map = wrap(plan.lay[0])
            self.lay_delta = torch.empty(B * 3 * (-(-self.Hc // N)) * (-(-self.Wc // N)), dtype=x.dtype, device=x.device)
            self.lopts = _lib.LayoutOpts(_lib.ptr(self.lay_map), N, None, _lib.ptr(self.lay_delta))
        if plan.order2:
            self.hist = torch.empty_like(x)                    # (written by every step before any step reads it: q[0] = 0)
            self.sopts = _lib.SolverOpts(None, _lib.ptr(self.hist))
        # (the second stream lets the library run coarse scales as two overlapping half-batches; same numbers either way)
        self.aux = _aux_stream(x.device) if d.two_streams else None

    def call(self, i0, k, seed, noise=None, sid0=0, seeds_dev=None, jump_noise=None, mix_dev=None):
        """Steps [i0, i0 + k) of the run: `noise` / `jump_noise` recorded draws of exactly these steps, or the in-kernel draws
        of `seeds_dev` (one seed per sample), of `mix_dev` ((B, K) int64 seeds, (B, K) float32 weights: a blend per sample)
        or of `seed`, at stream ids sid0 + 0 ... k - 1."""
        x, net, ref = self.x, self.net, (lambda o: C.byref(o) if o is not None else None)
        p = self.host = pack_steps(self.plan, i0, k)            # (the per-step host arrays of this piece)
        self.opts.noise = _lib.ptr(noise)
        for blk, name, v in ((self.kopts, "ab", p.ab), (self.ropts, "jumps", p.jumps), (self.ropts, "noise", _lib.ptr(jump_noise)),
                             (self.lopts, "g", p.g), (self.sopts, "q", p.q), (self.gopts, "thr", p.thr)):
            if blk is not None:
                setattr(blk, name, v)
        in_alt = C.c_int(0)
        args = [_lib.ptr(net.flat_params), _lib.ptr(self.packed), _lib.ptr(x), _lib.ptr(self.x_alt), _lib.ptr(self.eps),
                _lib.ptr(self.xt), p.coefs, p.tl, k, float(self.s), seed, sid0, net.dim_arg, x.shape[0], self.Hc, self.Wc,
                self.ws.data_ptr(), self.ws.numel(), _lib.stream_ptr(x.device), self.aux, C.byref(in_alt), C.byref(self.opts),
                *self.halo, ref(self.kopts), _lib.ptr(seeds_dev), ref(self.ropts), ref(self.lopts), ref(self.bopts)]
        mopts = _lib.MixOpts(_lib.ptr(mix_dev[0]), _lib.ptr(mix_dev[1]), int(mix_dev[0].shape[1])) if mix_dev is not None else None
        if self.gopts is not None:                             # (the gated run: the one entry that can say it)
            _lib.check(self.lib.sinddm_sample_chain_gate(*args, ref(self.sopts), ref(mopts), C.byref(self.gopts)),
                       "sinddm_sample_chain_gate")
        elif mix_dev is not None:                              # (the blended run: the one entry that can say it)
            _lib.check(self.lib.sinddm_sample_chain_mix(*args, ref(self.sopts), C.byref(mopts)), "sinddm_sample_chain_mix")
        elif self.sopts is not None:                           # (the multistep run: the one entry that can say it)
            _lib.check(self.lib.sinddm_sample_chain_solver(*args, C.byref(self.sopts)), "sinddm_sample_chain_solver")
        else:
            _lib.check(self.lib.sinddm_sample_chain_batch(*args), "sinddm_sample_chain_batch")
        if in_alt.value:
            self.x, self.x_alt = self.x_alt, self.x

    def centre(self, t: torch.Tensor) -> torch.Tensor:
        """The sample's own pixels of a (B, 3, H, W) buffer of the run's extended size (a view)."""
        hy, hx = self.halo
        return t[:, :, hy:hy + self.Hc, hx:hx + self.Wc]

    def result(self) -> torch.Tensor:
        return self.centre(self.x).contiguous() if self.tiled else self.x


class _KeepWindow:
    """The windows of one windowed known-region run of `MultiScaleGaussianDiffusion._run_steps` (`plan.window` set): `plan` /
    `img` are the run cropped to one (h, w) window per sample -- the steps of the full plan, every map gathered through the
    windows and therefore per-sample, the noise kind 'window' with its keys resolved -- which either route runs as it runs
    any plan; `fill` / `draw` make its draws, `leave` puts the result back into the full-size sample.  Gathers and the
    scatter are plain advanced indexing: they are outside the step loop."""

    def __init__(self, d, full, img):
        import copy
        self.d, self.full = d, full
        h, w, org = full.window
        B, Cc, H, W = (int(v) for v in img.shape)
        dev = img.device
        self.B, self.hw, self.HW, self.dev = B, (int(h), int(w)), (H, W), dev
        self.org = org.to(device=dev, dtype=torch.int32).contiguous()
        o = self.org.long()
        self.bi, self.ci = torch.arange(B, device=dev)[:, None, None, None], torch.arange(Cc, device=dev)[None, :, None, None]
        self.ys = (o[:, 0, None] + torch.arange(h, device=dev))[:, None, :, None]
        self.xs = (o[:, 1, None] + torch.arange(w, device=dev))[:, None, None, :]
        xt = full.xt
        if xt is not None and (xt.shape != img.shape or xt.dtype != img.dtype or xt.device != dev):
            raise _lib.SinddmError(f"img_prev_upsample {tuple(xt.shape)} {xt.dtype} {xt.device} does not match the "
                                   f"running sample {tuple(img.shape)} {img.dtype} {dev}")
        src = full.noise[1]
        if src is None:
            # an unseeded windowed run: every sample its own fresh 62-bit seed from torch's CPU generator
            src = ([[int(v)] for v in torch.randint(0, 2 ** 62, (B,), dtype=torch.int64).tolist()], None)
        self.keys, self.weights = src
        self.kd = torch.tensor(self.keys, dtype=torch.int64, device=dev)
        self.wd = torch.tensor(self.weights, dtype=torch.float32, device=dev) if self.weights is not None else None
        p = self.plan = copy.copy(full)
        p.win, p.noise = self, ("window", src)
        p.keep = (self.crop_plane(full.keep[0]), self.crop(full.keep[1]))
        p.roi = (self.crop_plane(full.roi[0]), self.crop(full.roi[1])) if full.roi is not None else None
        p.xt = self.crop(xt) if xt is not None else None
        p.per = (int(p.roi is not None), 1, 1, 0)
        self.img = self.crop(img)

    def crop(self, t):
        """(B, C, H, W) or a shared (C, H, W) -> the (B, C, h, w) windows."""
        t = t if t.dim() == 4 else t[None].expand((self.B,) + tuple(t.shape))
        return t[self.bi, self.ci, self.ys, self.xs].contiguous()

    def crop_plane(self, t):
        """(B, H, W) or a shared (H, W) -> the (B, h, w) windows."""
        t = t if t.dim() == 3 else t[None].expand((self.B,) + tuple(t.shape))
        return t[self.bi[:, 0], self.ys[:, 0], self.xs[:, 0]].contiguous()

    def fill(self, sids):
        """(len(sids), B, 3, h, w): slot i holds the windows of the run's draw at stream id sids[i] (one launch)."""
        lib, (h, w), (H, W) = _lib.load(), self.hw, self.HW
        ids = torch.tensor([int(v) for v in sids], dtype=torch.int64, device=self.dev)
        out = torch.empty((len(sids), self.B, 3, h, w), dtype=torch.float32, device=self.dev)
        _lib.check(lib.sinddm_normal_fill_window(_lib.ptr(out), len(sids), _lib.ptr(ids), self.B, H, W, _lib.ptr(self.org), h, w,
                                                 _lib.ptr(self.kd), _lib.ptr(self.wd), int(self.kd.shape[1]),
                                                 _lib.stream_ptr(self.dev)), "sinddm_normal_fill_window")
        return out

    def draw(self, kind, st):
        """The 'step' / 'jump' draw of step `st` on the step-by-step route (logged like `_draw` logs its draws)."""
        z = self.fill([noise_stream_id(self.plan.s, kind, st.pos)])[0]
        if self.d.draw_log is not None:
            self.d.draw_log.append((kind, int(self.plan.s), int(st.t), z.clone()))
        return z

    def leave(self, out):
        """The full-size result: the windows `out` inside, and outside what the full run leaves there -- every pixel out there
        is held (mask / hold level 1), so it is the kept value of the run's last step, ka * target + kb * z_last: the known
        image itself, bit for bit, when the run lands on the clean image; else the single-step keep entry on the last
        step's full-size draw under a mask of ones (the value does not depend on the network)."""
        d, full, B, (H, W) = self.d, self.full, self.B, self.HW
        last, kx = full.steps[-1], full.keep[1]
        if tuple(last.ab) == (1.0, 0.0) and last.k.mode != 1:
            res = (kx if kx.dim() == 4 else kx[None].expand(B, -1, -1, -1)).clone()
        else:
            lib = _lib.load()
            seeds, mix = ([k[0] for k in self.keys], None) if self.weights is None else (None, (self.keys, self.weights))
            z = d._keyed_normal(seeds, mix, (B, 3, H, W), noise_stream_id(full.s, "step", last.pos), self.dev)
            zero, ones, res = torch.zeros_like(z), torch.ones((H, W), dtype=z.dtype, device=self.dev), torch.empty_like(z)
            rows = [slice(b, b + 1) for b in range(B)] if kx.dim() == 4 else [slice(0, B)]
            for r in rows:
                xt = full.xt[r] if full.xt is not None else None
                _lib.check(lib.sinddm_reverse_step_keep(_lib.ptr(zero[r]), _lib.ptr(zero[r]), _lib.ptr(xt), _lib.ptr(z[r]),
                                                        _lib.ptr(res[r]), C.byref(last.k), None, None, _lib.ptr(ones),
                                                        _lib.ptr(kx[r.start] if kx.dim() == 4 else kx), *last.ab,
                                                        r.stop - r.start, 3, H * W, _lib.stream_ptr(self.dev)),
                           "sinddm_reverse_step_keep")
        res[self.bi, self.ci, self.ys, self.xs] = out
        return res


class MultiScaleGaussianDiffusion(nn.Module):
    """Multi-scale DDPM with SinDDM's re-blurring (reference SinDDM/models.py:155-631)."""

    def __init__(self, denoise_fn, *, save_interm=False, results_folder='/Results', n_scales, scale_factor,
                 image_sizes, scale_mul=(1, 1), channels=3, timesteps=100, train_full_t=False, scale_losses=None,
                 loss_factor=1, loss_type='l1', betas=None, device=None, reblurring=True, sample_limited_t=False,
                 omega=0):
        super().__init__()
        self.device = device
        self.save_interm = save_interm
        self.results_folder = Path(results_folder)
        self.channels = channels
        self.n_scales = n_scales
        self.scale_factor = scale_factor
        self.scale_mul = scale_mul
        self.sample_limited_t = sample_limited_t
        self.reblurring = reblurring
        self.img_prev_upsample = None

        # guided-sampling state of the reference (models.py:193-220).  CLIP itself (clip/, text2live_util/) is outside
        # the hot-path build; the guidance BRANCH of p_mean_variance (models.py:367-431) is implemented against the
        # interface the reference uses: `clip_model` is any object with zero_grad() and a differentiable
        # calculate_clip_loss(image in [0,1], text_embedds) -> scalar (stock PyTorch-ROCm autograd).
        self.guidance_sub_iters = None
        self.stop_guidance = None
        self.quantile = 0.8
        self.clip_model = None
        self.clip_strength = None
        self.clip_text = ''
        self.text_embedds = None
        self.text_embedds_hr = None
        self.text_embedds_lr = None
        self.clip_text_features = None
        self.clip_score = []
        self.clip_mask = None
        self.llambda = 0
        self.x_recon_prev = None
        self.clip_roi_bb = []
        self.omega = omega
        self.roi_bbs = []
        self.roi_bbs_stat = []
        self.roi_target_patch = []
        self._roi_cache = {}

        # (W,H) -> (H,W)   models.py:222-223
        self.image_sizes = tuple((image_sizes[i][1], image_sizes[i][0]) for i in range(n_scales))
        self.denoise_fn = denoise_fn

        if exists(betas):
            betas = betas.detach().cpu().numpy() if isinstance(betas, torch.Tensor) else betas
        else:
            betas = cosine_beta_schedule(timesteps)
        alphas = 1. - betas
        abar = np.cumprod(alphas, axis=0)
        abar_prev = np.append(1., abar[:-1])
        timesteps, = betas.shape
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        f32 = partial(torch.tensor, dtype=torch.float32)
        reg = self.register_buffer
        reg('betas', f32(betas))
        reg('alphas_cumprod', f32(abar))
        reg('alphas_cumprod_prev', f32(abar_prev))
        reg('sqrt_alphas_cumprod', f32(np.sqrt(abar)))
        reg('sqrt_one_minus_alphas_cumprod', f32(np.sqrt(1. - abar)))
        reg('log_one_minus_alphas_cumprod', f32(np.log(1. - abar)))
        reg('sqrt_recip_alphas_cumprod', f32(np.sqrt(1. / abar)))
        reg('sqrt_recipm1_alphas_cumprod', f32(np.sqrt(1. / abar - 1)))
        post_var = betas * (1. - abar_prev) / (1. - abar)
        reg('posterior_variance', f32(post_var))
        reg('posterior_log_variance_clipped', f32(np.log(np.maximum(post_var, 1e-20))))
        reg('posterior_mean_coef1', f32(betas * np.sqrt(abar_prev) / (1. - abar)))
        reg('posterior_mean_coef2', f32((1. - abar_prev) * np.sqrt(alphas) / (1. - abar)))

        # per-scale starting timesteps (bit-exact integer bookkeeping, models.py:269-280)
        sigma_t = np.sqrt(1. - abar) / np.sqrt(abar)
        self.num_timesteps_trained = [self.num_timesteps]
        self.num_timesteps_ideal = [self.num_timesteps]
        if scale_losses is not None:
            for i in range(n_scales - 1):
                self.num_timesteps_ideal.append(int(np.argmax(sigma_t > loss_factor * scale_losses[i])))
                self.num_timesteps_trained.append(int(timesteps) if train_full_t else self.num_timesteps_ideal[i + 1])
        # gamma blur schedule (models.py:283-287): float64 ratio, clamped, stored fp32
        gammas = torch.zeros((n_scales - 1, self.num_timesteps), dtype=torch.float32)
        for i in range(n_scales - 1):
            gammas[i, :] = (torch.tensor(sigma_t) / (loss_factor * scale_losses[i])).clamp(min=0, max=1)
        reg('gammas', gammas)
        if device is not None:
            # the reference builds `gammas` directly on `device`; mirror that placement
            self.gammas = self.gammas.to(device)

        self._host_tabs: Optional[dict] = None
        self._host_ver = None
        # tileable TRAINING: (wrap_y, wrap_x) -- p_losses trains the network with circular padding on the wrapped axes, by
        # the same construction (x_noisy extended by its wrapped halo, the loss on the centre: every parameter gradient is
        # then the circularly padded network's).  Separate from `tile`, which p_losses does not read; not
        # stored in checkpoints.  Read by train_step.TrainStep (its `halo`), like `train_weights` below.
        self.train_tile = (False, False)
        # masked training (no reference counterpart): None, or one (h,w) fp32 map per scale on the training device, finite and
        # >= 0.  p_losses then takes sum(w e) / (B C sum w) instead of the mean over every pixel, e the loss type's
        # per-element error: where w == 0 the image never reaches the weights -- and, the receptive field being a square of
        # Chebyshev radius SINDDM_TILE_HALO, with w == 0 within that distance of a hole the weights provably never see what
        # the hole contains (functions.train_weight_pyramid builds such maps).  A defective map is refused by
        # train_step.TrainStep before the step launches anything.  Replace the list entry to change a map (the normaliser is
        # cached per scale and map object: {s: (map, float64 sum)}, a plain attribute).  Not stored in checkpoints.
        self.train_weights = None
        self._train_weight_norm = {}
        # crop training (no reference counterpart): None, or (ch, cw) -- at every scale larger than that, each
        # sample of a p_losses batch sees its own (min(ch,H), min(cw,W)) window of x_start / x_orig, the network runs on the
        # windows, and the loss is taken on each window minus `train_crop_margin` rows / columns along every side that is not
        # an image border.  With a margin >= SINDDM_TILE_HALO the step equals full-image masked steps (the statement of
        # DESIGN.md 4).  The origins: p_losses' `windows` argument, else `crop_fn(crop_step, s, B) -> (B,2)` (the trainer sets
        # `crop_step` to its step), else the clamped draw of functions.crop_windows from a private CPU generator seeded
        # torch.initial_seed() + rank on first use.  Not together with `train_tile`; not stored in checkpoints.
        self.train_crop = None
        self.train_crop_margin = 0
        self.crop_fn = None
        self.crop_step = 0
        self._crop_gen = None
        self._train_crop_sat = {}
        # the sampling options: sampler.sampling_defaults lists and describes them, `sampling()` below sets them for a block
        for name, value in sampling_defaults().items():
            setattr(self, name, value)

    def sampling(self, **options):
        """Context manager: the sampling options `options` (names of sampler.sampling_defaults; any other name is a TypeError
        before anything is set) for the length of the block, which is handed this model.  On the way out, by return or by
        exception, every named attribute is the very object it was on the way in -- not a copy, not the default.  Scopes
        nest.  No value is looked at: the readers of the options validate, as ever, when a run starts."""
        unknown = sorted(set(options) - SAMPLING_OPTIONS)
        if unknown:
            raise TypeError(f"sampling(): {', '.join(unknown)}: not a sampling option (sampler.sampling_defaults)")

        @contextmanager
        def scope():
            found = {name: getattr(self, name) for name in options}
            for name, value in options.items():
                setattr(self, name, value)
            try:
                yield self
            finally:
                for name, value in found.items():
                    setattr(self, name, value)
        return scope()

    # ---- host copies of the per-t tables (scalar kernel arguments; no device sync per step) ----
    _TABS = ('alphas_cumprod', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod',
             'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_log_variance_clipped',
             'posterior_mean_coef1', 'posterior_mean_coef2', 'gammas')

    def _host(self) -> dict:
        ver = tuple(getattr(self, n)._version for n in self._TABS) + tuple(getattr(self, n).data_ptr() for n in self._TABS)
        if self._host_tabs is None or ver != self._host_ver:
            h = {n: getattr(self, n).detach().cpu().numpy().astype(np.float32) for n in self._TABS}
            h['gammas_clamped'] = np.clip(h['gammas'], np.float32(0), np.float32(0.55))     # models.py:314,358
            h['sigma_plain'] = np.exp(np.float32(0.5) * h['posterior_log_variance_clipped']).astype(np.float32)
            self._host_tabs, self._host_ver = h, ver
        return self._host_tabs

    def _seeds_for(self, s: int, B: int):
        """The B seeds of scale s from `sample_seeds` (validated), or None when unset."""
        ss = self.sample_seeds
        if ss is None:
            return None
        if self.seed_mix is not None:
            raise ValueError("sample_seeds and seed_mix are both set: two noise sources")
        if self.noise_fn is not None:
            raise ValueError("sample_seeds and noise_fn are both set: two noise sources")
        if isinstance(ss, (torch.Tensor, np.ndarray)):
            ss = ss.tolist()
        ss = list(ss)
        if len(ss) > 0 and isinstance(ss[0], (list, tuple, np.ndarray, torch.Tensor)):
            if len(ss) != self.n_scales:
                raise ValueError(f"sample_seeds has {len(ss)} rows for {self.n_scales} scales")
            row = ss[min(int(s), self.n_scales - 1)]        # (custom sizes past the pyramid sample with the finest scale's row)
            row = row.tolist() if isinstance(row, (np.ndarray, torch.Tensor)) else list(row)
        else:
            row = ss
        if len(row) != int(B):
            raise ValueError(f"sample_seeds holds {len(row)} seeds for a batch of {int(B)}")
        return _check_seed_row(row)

    def _mix_for(self, s: int, B: int):
        """The (keys, weights) tables of scale s from `seed_mix` (validated, [B][K] each), or None when unset."""
        mx = self.seed_mix
        if mx is None:
            return None
        if self.sample_seeds is not None:
            raise ValueError("seed_mix and sample_seeds are both set: two noise sources")
        if self.noise_fn is not None:
            raise ValueError("seed_mix and noise_fn are both set: two noise sources")
        refuse(self, "seed_mix", "clip")
        if not isinstance(mx, (tuple, list)) or len(mx) != 2:
            raise ValueError("seed_mix is a pair (keys, weights)")
        keys, w = (v.tolist() if isinstance(v, (np.ndarray, torch.Tensor)) else list(v) for v in mx)

        def depth(v):
            return 1 + depth(v[0]) if isinstance(v, (list, tuple, np.ndarray, torch.Tensor)) and len(v) > 0 else 0
        if depth(keys) != depth(w) or depth(keys) not in (2, 3):
            raise ValueError("seed_mix: keys and weights are [B][K] or [n_scales][B][K] nested sequences of one shape")
        if depth(keys) == 3:
            if len(keys) != self.n_scales or len(w) != self.n_scales:
                raise ValueError(f"seed_mix has {len(keys)} / {len(w)} tables for {self.n_scales} scales")
            i = min(int(s), self.n_scales - 1)                # (custom sizes past the pyramid sample with the finest scale's table)
            keys, w = keys[i], w[i]
        if len(keys) != int(B) or len(w) != int(B):
            raise ValueError(f"seed_mix holds {len(keys)} rows for a batch of {int(B)}")
        return _check_mix(keys, w)

    @staticmethod
    def _mix_tensors(mix, device):
        """The device tables of a validated mix: (B, K) int64 seeds, (B, K) float32 weights."""
        return (torch.tensor(mix[0], dtype=torch.int64, device=device), torch.tensor(mix[1], dtype=torch.float32, device=device))

    def _keyed_normal(self, seeds, mix, shape, sid: int, device) -> torch.Tensor:
        """(B, ...) N(0,1) of a seeded run: slice b = sinddm_normal_fill(numel per sample, seeds[b], sid) -- or, with a `mix`,
        the blend of those of keys[b][k]."""
        lib = _lib.load()
        shape = tuple(int(v) for v in shape)
        z = torch.empty(shape, dtype=torch.float32, device=device)
        n, st = z.numel() // shape[0], _lib.stream_ptr(z.device)
        if mix is not None:
            kd, wd = self._mix_tensors(mix, device)
            _lib.check(lib.sinddm_normal_fill_mix(_lib.ptr(z), shape[0], n, _lib.ptr(kd), _lib.ptr(wd), int(kd.shape[1]), int(sid), st),
                       "sinddm_normal_fill_mix")
        else:
            sd = torch.tensor(seeds, dtype=torch.int64, device=device)
            _lib.check(lib.sinddm_normal_fill_samples(_lib.ptr(z), shape[0], n, _lib.ptr(sd), int(sid), st), "sinddm_normal_fill_samples")
        return z

    def _draw(self, kind: str, shape, s: int, t: int, device, pos: int = 0) -> torch.Tensor:
        """One N(0,1) draw of the sampler: `kind` 'init' / 'renoise' / 'step' / 'jump' (`pos` = the step's position in its
        run; 'jump' is the second draw of the jump that follows that step)."""
        seeds = self._seeds_for(s, shape[0])
        mix = self._mix_for(s, shape[0])
        if seeds is not None or mix is not None:
            # (a blend is drawn like its seeds would be: same stream ids, same extended size, the blend of the slices)
            # the tiled chain draws over the EXTENDED sample and discards the halo's draws: take the centre
            hy, hx = self._tile_halo() if kind in ("step", "jump") else (0, 0)
            H, W = int(shape[-2]), int(shape[-1])
            z = self._keyed_normal(seeds, mix, tuple(shape[:-2]) + (H + 2 * hy, W + 2 * hx), noise_stream_id(s, kind, pos), device)
            if hy or hx:
                z = z[..., hy:hy + H, hx:hx + W].contiguous()
        elif self.noise_fn is not None:
            return self.noise_fn(kind, tuple(shape), int(s), int(t), device).contiguous()
        else:
            z = torch.randn(tuple(shape), device=device)
        if self.draw_log is not None:
            self.draw_log.append((kind, int(s), int(t), z.clone()))
        return z

    def step_coefs(self, t: int, s: int, clip_denoised: bool = True) -> _lib.StepCoefs:
        """Host scalars of one reverse step (everything `extract` gathers in models.py:306-352)."""
        h = self._host()
        t = int(t)
        k = _lib.StepCoefs()
        k.clip = 1 if clip_denoised else 0
        k.sqrt_recip_ac_t = float(h['sqrt_recip_alphas_cumprod'][t])
        k.sqrt_recipm1_ac_t = float(h['sqrt_recipm1_alphas_cumprod'][t])
        one = np.float32(1)
        if (not self.reblurring) or int(s) == 0:
            k.mode = 0
            k.coef1_t = float(h['posterior_mean_coef1'][t])
            k.coef2_t = float(h['posterior_mean_coef2'][t])
            k.sigma = float(h['sigma_plain'][t]) if t != 0 else 0.0
            return k
        g = h['gammas_clamped'][int(s) - 1]
        k.gamma_t = float(g[t])
        if t > 0:
            k.mode = 1
            k.gamma_tm1 = float(g[t - 1])
            ac_tm1 = h['alphas_cumprod'][t - 1]
            var = np.float32(np.float32(self.omega) * (one - ac_tm1))                       # models.py:335-337
            logvar = np.log(np.maximum(var, np.float32(1e-20)))
            k.sqrt_ac_tm1 = float(h['sqrt_alphas_cumprod'][t - 1])
            k.sqrt_ac_t = float(h['sqrt_alphas_cumprod'][t])
            k.sqrt_1m_ac_t = float(h['sqrt_one_minus_alphas_cumprod'][t])
            k.sqrt_1m_ac_tm1_mvar = float(np.sqrt(np.float32(one - ac_tm1 - var)))
            k.sigma = float(np.exp(np.float32(0.5) * np.float32(logvar)))
        else:
            k.mode = 2
            k.sigma = 0.0
        return k

    def step_coefs_to(self, t: int, u: int, s: int, clip_denoised: bool = True, eta: float = 1.0) -> _lib.StepCoefs:
        """Host scalars of the reverse step from level t that lands on level u < t (u = -1: the clean image), in the fields of
        `step_coefs`, so that every step kernel takes the strided step unchanged.  u == t - 1 with eta == 1 IS
        `step_coefs(t, s)`.  Mode 0 (float64 on the tables of `_jump_levels`): the DDIM step with
        sigma = eta * sqrt((1 - ac_u) / (1 - ac_t)) * sqrt(1 - ac_t / ac_u), coef2 = sqrt(sb_u^2 - sigma^2) / sb_t,
        coef1 = sa_u - coef2 * sa_t; landing clean coef1 = 1, coef2 = sigma = 0.  Mode 1: the `tm1` fields take level u
        (var = omega * (1 - ac_u)); landing clean at a scale > 0 is mode 2 with t's own scalars.  `eta` acts in mode 0 only."""
        t, u, s = int(t), int(u), int(s)
        if not (0 <= t < self.num_timesteps and -1 <= u < t):
            raise ValueError(f"step_coefs_to: no step from level {t} to level {u}")
        if u == t - 1 and float(eta) == 1.0:
            return self.step_coefs(t, s, clip_denoised)
        h = self._host()
        k = _lib.StepCoefs()
        k.clip = 1 if clip_denoised else 0
        k.sqrt_recip_ac_t = float(h['sqrt_recip_alphas_cumprod'][t])
        k.sqrt_recipm1_ac_t = float(h['sqrt_recipm1_alphas_cumprod'][t])
        one = np.float32(1)
        if (not self.reblurring) or s == 0:
            k.mode = 0
            if u < 0:
                k.coef1_t, k.coef2_t, k.sigma = 1.0, 0.0, 0.0
                return k
            sa, sb, _ = self._jump_levels(s)
            ac = h['alphas_cumprod'].astype(np.float64)
            sigma = float(eta) * np.sqrt((1.0 - ac[u]) / (1.0 - ac[t])) * np.sqrt(max(0.0, 1.0 - ac[t] / ac[u]))
            coef2 = np.sqrt(max(0.0, sb[u] * sb[u] - sigma * sigma)) / sb[t]
            k.coef1_t, k.coef2_t, k.sigma = float(sa[u] - coef2 * sa[t]), float(coef2), float(sigma)
            return k
        g = h['gammas_clamped'][s - 1]
        k.gamma_t = float(g[t])
        if u < 0:
            k.mode = 2
            k.sigma = 0.0
            return k
        k.mode = 1
        k.gamma_tm1 = float(g[u])
        ac_u = h['alphas_cumprod'][u]
        var = np.float32(np.float32(self.omega) * (one - ac_u))
        logvar = np.log(np.maximum(var, np.float32(1e-20)))
        k.sqrt_ac_tm1 = float(h['sqrt_alphas_cumprod'][u])
        k.sqrt_ac_t = float(h['sqrt_alphas_cumprod'][t])
        k.sqrt_1m_ac_t = float(h['sqrt_one_minus_alphas_cumprod'][t])
        k.sqrt_1m_ac_tm1_mvar = float(np.sqrt(np.float32(one - ac_u - var)))
        k.sigma = float(np.exp(np.float32(0.5) * np.float32(logvar)))
        return k

    def _kappa(self, s: int) -> np.ndarray:
        """float64 kappa[l] = sa[l] * (1 - gamma[l]) / sb[l] per level of scale s (the tables of `_jump_levels`): the variable
        the probability flow of SinDDM's blurred process is linear in; it rises as the level falls."""
        sa, sb, g = self._jump_levels(s)
        return sa * (1.0 - g) / sb

    def _solver_q(self, s: int, taus, lands):
        """The multistep factors q_i = rho_i * kappa[tau_i] of a run (float64; sinddm_solver_opts): rho_i =
        ln(kappa[u_i] / kappa[tau_i]) / (2 ln(kappa[tau_i] / kappa[tau_{i-1}])), 0 on the first step and on a step that lands on
        the clean image.  kappa[tau] = (1 - gamma[tau]) / sqrt_recipm1_ac[tau]."""
        kap = self._kappa(s)
        q = []
        for i, (t, u) in enumerate(zip(taus, lands)):
            if i == 0 or u < 0:
                q.append(0.0)
                continue
            rho = np.log(kap[u] / kap[t]) / (2.0 * np.log(kap[t] / kap[taus[i - 1]]))
            q.append(float(rho * kap[t]))
        return q

    def _few_step_cfg(self, s: int):
        """(n or None, spacing, order) of the few-step options for scale s, validated; None when every one is at its default."""
        order, spacing, eta = int(self.solver_order), self.sample_spacing, float(self.eta)
        if order not in (1, 2):
            raise ValueError(f"solver_order = {self.solver_order!r}: 1 or 2")
        if spacing not in ('t', 'logsnr'):
            raise ValueError(f"sample_spacing = {spacing!r}: 't' or 'logsnr'")
        if not 0.0 <= eta:
            raise ValueError(f"eta = {self.eta!r} must be >= 0")
        n = self.sample_steps
        if n is not None and not isinstance(n, (int, np.integer)):
            n = list(n)
            if len(n) != self.n_scales:
                raise ValueError(f"sample_steps has {len(n)} entries for {self.n_scales} scales")
            n = n[min(int(s), self.n_scales - 1)]              # (custom sizes past the pyramid take the finest scale's entry)
        if n is not None:
            n = int(n)
            if n < 1:
                raise ValueError(f"sample_steps = {self.sample_steps!r}: at least one evaluation per scale")
        if self.sample_steps is None and order == 1 and eta == 1.0:
            return None
        refuse(self, "few_step", "clip")
        refuse(self, "few_step", "resample")
        return n, spacing, order

    # ---- reference API: fine-grained pieces (off the hot path; kept for callers / app modes) ----
    def q_mean_variance(self, x_start, t):                                  # models.py:300-304
        mean = extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        variance = extract(1. - self.alphas_cumprod, t, x_start.shape)
        log_variance = extract(self.log_one_minus_alphas_cumprod, t, x_start.shape)
        return mean, variance, log_variance

    def predict_start_from_noise(self, x_t, t, s, noise):                   # models.py:306-318
        x0 = extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - extract(
            self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise
        if not self.reblurring or s == 0:
            return x0, x0
        g = extract(self.gammas[s - 1].reshape(-1).clamp(0, 0.55), t, x0.shape)
        return (x0 - g * self.img_prev_upsample) / (1 - g), x0

    def q_posterior(self, x_start, x_t_mix, x_t, t, s):                     # models.py:321-352
        if not self.reblurring or s == 0:
            mean = extract(self.posterior_mean_coef1, t, x_t.shape) * x_start + extract(
                self.posterior_mean_coef2, t, x_t.shape) * x_t
            var = extract(self.posterior_variance, t, x_t.shape)
            logvar = extract(self.posterior_log_variance_clipped, t, x_t.shape)
        elif t[0] > 0:
            var = self.omega * (1 - extract(self.alphas_cumprod, t - 1, x_t.shape)) + torch.zeros_like(x_t)
            logvar = torch.log(var.clamp(1e-20, None))
            mean = extract(self.sqrt_alphas_cumprod, t - 1, x_t.shape) * x_start + torch.sqrt(
                1 - extract(self.alphas_cumprod, t - 1, x_t.shape) - var) * (
                x_t - extract(self.sqrt_alphas_cumprod, t, x_t.shape) * x_t_mix) / extract(
                self.sqrt_one_minus_alphas_cumprod, t, x_t.shape)
        else:
            mean = x_start
            var = extract(self.posterior_variance, t, x_t.shape)
            logvar = extract(self.posterior_log_variance_clipped, t, x_t.shape)
        return mean, var, logvar

    def roi_patch_modification(self, x_recon, scale=0, eta=0.8):            # models.py:291-298 (in place, like it)
        w, c = self.roi_edit_maps(scale, x_recon.shape[-2], x_recon.shape[-1], x_recon.device, eta)
        if w.dim() == 3:                                                    # per-sample maps (roi_bbs_batch)
            if w.shape[0] != x_recon.shape[0]:
                raise ValueError(f"roi_bbs_batch has {w.shape[0]} box lists, the batch {x_recon.shape[0]} samples")
            x_recon.mul_(w[:, None]).add_(c)
            return x_recon
        x_recon.mul_(w[None, None]).add_(c[None])
        return x_recon

    def roi_edit_maps(self, scale: int, H: int, W: int, device, eta: float = 0.8):
        """The reference's sequential ROI blends `x[box] = eta * patch + (1 - eta) * x[box]` over all boxes
        (models.py:291-298) composed into ONE per-pixel affine map x -> w * x + c (w: (H,W), c: (3,H,W)); this is
        what the step kernels apply (`sinddm_sample_chain_ex` with edit maps; `sinddm_reverse_step_edit` on the
        step-by-step route).  Cached per (scale, size, boxes).  With `roi_bbs_batch` set the maps are per sample,
        (B,H,W) and (B,3,H,W): row b is built from roi_bbs_batch[b] (and roi_target_patch_batch[b]) exactly as the shared
        pair is built from `roi_bbs`."""
        boxes = lambda bbs: tuple(tuple(int(v) for v in bb) for bb in bbs)
        if self.roi_bbs_batch is not None:
            pb = self.roi_target_patch_batch
            if pb is not None and len(pb) != len(self.roi_bbs_batch):
                raise ValueError(f"roi_target_patch_batch has {len(pb)} entries, roi_bbs_batch {len(self.roi_bbs_batch)}")
            patches = [(pb[b] if pb is not None else self.roi_target_patch)[scale] for b in range(len(self.roi_bbs_batch))]
            key = (int(scale), int(H), int(W), float(eta), tuple(boxes(bbs) for bbs in self.roi_bbs_batch),
                   tuple(id(pt) for pt in patches))
            if self._roi_cache.get("key") == key:
                return self._roi_cache["w"], self._roi_cache["c"]
            rows = [self._roi_maps_one(scale, H, W, device, eta, bbs, pt) for bbs, pt in zip(self.roi_bbs_batch, patches)]
            self._roi_cache = {"key": key, "w": torch.stack([r[0] for r in rows]).contiguous(),
                               "c": torch.stack([r[1] for r in rows]).contiguous()}
            return self._roi_cache["w"], self._roi_cache["c"]
        key = (int(scale), int(H), int(W), float(eta), boxes(self.roi_bbs), id(self.roi_target_patch[scale]))
        if self._roi_cache.get("key") == key:
            return self._roi_cache["w"], self._roi_cache["c"]
        w, c = self._roi_maps_one(scale, H, W, device, eta, self.roi_bbs, self.roi_target_patch[scale])
        self._roi_cache = {"key": key, "w": w.contiguous(), "c": c.contiguous()}
        return self._roi_cache["w"], self._roi_cache["c"]

    def _roi_maps_one(self, scale: int, H: int, W: int, device, eta: float, bbs, target_patch):
        """(w, c) of one box list and the scale's target patch: one job's maps."""
        w = torch.ones((H, W), device=device, dtype=torch.float32)
        c = torch.zeros((self.channels, H, W), device=device, dtype=torch.float32)
        for bb in bbs:                                                      # bounding box is [y, x, h, w]
            bb = [int(bb_i / np.power(self.scale_factor, self.n_scales - scale - 1)) for bb_i in bb]
            y, x, h, ww = bb
            patch = F.interpolate(target_patch.to(device=device, dtype=torch.float32), size=(h, ww))[0]
            c[:, y:y + h, x:x + ww] = eta * patch + (1 - eta) * c[:, y:y + h, x:x + ww]
            w[y:y + h, x:x + ww] *= (1 - eta)
        return w, c

    def _clip_guidance(self, x_recon, t0: int, s: int, clip_denoised: bool):
        """The CLIP-guidance block of p_mean_variance (models.py:367-421): the score's gradient is taken with respect to
        x_recon itself (a leaf -- nothing flows back through the network), soft-thresholded into a mask at the first
        call, normalised to the image's norm inside the mask and added; changes of the previous step are blended in
        with `llambda`.  Runs on stock PyTorch autograd: `clip_model` is external (see __init__)."""
        from .functions import thresholded_grad
        if clip_denoised:
            x_recon = x_recon.clamp(-1., 1.)
        if self.clip_mask is not None:
            x_recon = x_recon * (1 - self.clip_mask) + (
                (1 - self.llambda) * self.x_recon_prev + self.llambda * x_recon) * self.clip_mask
        x_recon = x_recon.detach().requires_grad_(True)
        emb = self.text_embedds_hr if s > 0 else self.text_embedds_lr
        with torch.enable_grad():
            for i in range(self.guidance_sub_iters[s]):
                self.clip_model.zero_grad()
                score = -self.clip_model.calculate_clip_loss((x_recon + 1) * 0.5, emb)
                clip_grad = torch.autograd.grad(score, x_recon, create_graph=False)[0]
                if self.clip_mask is None:
                    clip_grad, clip_mask = thresholded_grad(grad=clip_grad, quantile=self.quantile)
                    self.clip_mask = clip_mask.float()
                if self.save_interm:                                        # models.py:394-404
                    self._dump_interm(self.clip_mask.to(torch.float64), s, f'clip_mask_s-{s}.png', renorm=False)
                    self._dump_interm(x_recon.detach().clamp(-1., 1.), s, f'clip_out_s-{s}_t-{t0}_subiter_{i}.png')
                with torch.no_grad():
                    division_norm = torch.linalg.vector_norm(x_recon * self.clip_mask, dim=(1, 2, 3), keepdim=True) / \
                        torch.linalg.vector_norm(clip_grad * self.clip_mask, dim=(1, 2, 3), keepdim=True)
                    x_recon += self.clip_strength * division_norm * clip_grad * self.clip_mask
                    x_recon.clamp_(-1., 1.)
                self.clip_score.append(score.detach().cpu())
        self.x_recon_prev = x_recon.detach()
        return self.x_recon_prev.clone()

    def _clip_active(self, t0: int, s: int) -> bool:                        # the condition of models.py:368
        return bool(self.clip_guided_sampling and (self.stop_guidance <= t0 or s < self.n_scales - 1)
                    and self.guidance_sub_iters[s] > 0)

    def p_mean_variance(self, x, t, s, clip_denoised: bool):               # models.py:354-447
        with torch.no_grad():
            eps = self._eps(x, t, int(t[0]), s)
            x_recon, x_t_mix = self.predict_start_from_noise(x, t=t, s=s, noise=eps)
            if self.save_interm:                                            # models.py:360-366
                self._dump_x_recon(x_recon, int(t[0]), int(s))
        if self._clip_active(int(t[0]), int(s)):                            # models.py:367-421
            x_recon = self._clip_guidance(x_recon, int(t[0]), int(s), clip_denoised)
        elif self.roi_guided_sampling and (s < self.n_scales - 1):         # models.py:430-431
            x_recon = self.roi_patch_modification(x_recon, scale=s)
        with torch.no_grad():
            if int(s) > 0 and t[0] > 0 and self.reblurring:
                g = extract(self.gammas[s - 1].reshape(-1).clamp(0, 0.55), t - 1, x_recon.shape)
                x_tm1_mix = g * self.img_prev_upsample + (1 - g) * x_recon
            else:
                x_tm1_mix = x_recon
            if clip_denoised:
                x_tm1_mix = x_tm1_mix.clamp(-1., 1.)
                x_t_mix = x_tm1_mix if ((not self.reblurring) or s == 0) else x_t_mix.clamp(-1., 1.)
            return self.q_posterior(x_start=x_tm1_mix, x_t_mix=x_t_mix, x_t=x, t=t, s=s)

    def _p_sample_guided(self, x, t_host: int, s: int, clip_denoised: bool, repeat_noise: bool, step_pos: int = 0):
        """p_sample (models.py:449-459) through p_mean_variance in eager torch ops: the path of CLIP-guided steps (the
        fused reverse-step kernel has no place for an external autograd call between x_recon and the posterior)."""
        t = torch.full((x.shape[0],), int(t_host), device=x.device, dtype=torch.long)
        mean, _, logvar = self.p_mean_variance(x=x, t=t, s=s, clip_denoised=clip_denoised)
        if repeat_noise:
            z = noise_like(x.shape, x.device, True)
        else:
            z = self._draw("step", x.shape, s, t_host, x.device, step_pos)
        nonzero = 0.0 if t_host == 0 else 1.0
        return mean + nonzero * (0.5 * logvar).exp() * z

    # ---- hot path -----------------------------------------------------------------------------
    def _coef_table(self, s: int, clip_denoised: bool = True):
        """`step_coefs` of every t of scale s as one ctypes array (built once per schedule / reblurring / omega)."""
        key = (int(s), bool(clip_denoised), bool(self.reblurring), float(self.omega))
        self._host()                                             # refreshes self._host_ver
        cache = getattr(self, "_coef_cache", None)
        if cache is None or cache.get("ver") != self._host_ver:
            cache = {"ver": self._host_ver}
            self._coef_cache = cache
        tab = cache.get(key)
        if tab is None:
            tab = (_lib.StepCoefs * self.num_timesteps)(*[self.step_coefs(t, s, clip_denoised)
                                                          for t in range(self.num_timesteps)])
            cache[key] = tab
        return tab

    def _keep_ab_table(self) -> np.ndarray:
        """(T, 2) fp32: row t = (keep_a, keep_b) of the step t -> t-1, the forward scalars of the known image at t-1:
        (sqrt_alphas_cumprod[t-1], sqrt_one_minus_alphas_cumprod[t-1]) for t > 0 and (1, 0) for t == 0."""
        h = self._host()
        cache = getattr(self, "_keep_ab_cache", None)
        if cache is None or cache[0] != self._host_ver:
            ab = np.empty((self.num_timesteps, 2), dtype=np.float32)
            ab[0] = (1.0, 0.0)
            ab[1:, 0] = h['sqrt_alphas_cumprod'][:-1]
            ab[1:, 1] = h['sqrt_one_minus_alphas_cumprod'][:-1]
            cache = (self._host_ver, ab)
            self._keep_ab_cache = cache
        return cache[1]

    def _jump_levels(self, s: int):
        """float64 (sa, sb, gamma) per noise level of scale s, as the jumps see the process: sa / sb = sqrt(ac) / sqrt(1 - ac)
        of the host copy of `alphas_cumprod` (so that sa^2 + sb^2 = 1 to float64 rounding), gamma the clamped sampling gamma
        (the row `gamma_t` / `gamma_tm1` of `step_coefs` come from; zeros in mode 0)."""
        h = self._host()
        ac = h['alphas_cumprod'].astype(np.float64)
        if (not self.reblurring) or int(s) == 0:
            g = np.zeros_like(ac)
        else:
            g = h['gammas_clamped'][int(s) - 1].astype(np.float64)
        return np.sqrt(ac), np.sqrt(1.0 - ac), g

    def _jump_table(self, s: int):
        """jt(l, l2) -> (r, s, d) in float64 of the jump from level l up to level l2 >= l at scale s (sinddm_jump_coefs):
        r = sa[l2] / sa[l], s = sqrt(1 - r^2), d = sa[l2] * (gamma[l2] - gamma[l])."""
        sa, _, g = self._jump_levels(s)

        def jt(l: int, l2: int):
            l, l2 = int(l), int(l2)
            if not 0 <= l <= l2 < self.num_timesteps:
                raise ValueError(f"jump {l} -> {l2} outside the schedule's levels")
            r = float(sa[l2] / sa[l])
            return r, float(np.sqrt(max(0.0, 1.0 - r * r))), float(sa[l2] * (g[l2] - g[l]))
        return jt

    def _resample_cfg(self):
        """(R, J) of `resample` (validated) when it asks for jumps, else None."""
        if self.resample is None:
            return None
        R, J = (int(v) for v in self.resample)
        if R < 1 or J < 1:
            raise ValueError(f"resample = {self.resample!r}: R and J must be >= 1")
        refuse(self, "resample", "clip")
        return (R, J) if R > 1 else None

    def _keep_entry(self, s: int, img: torch.Tensor):
        """The (mask, x0) pair of `keep_maps` for scale s, checked against the running sample (the library takes raw
        pointers: a mismatching map would be read out of bounds), or None.  Either may carry a leading batch dimension,
        which must be the running batch."""
        if self.keep_maps is None:
            return None
        refuse(self, "keep_maps", "clip")
        entry = self.keep_maps.get(int(s))
        if entry is None:
            return None
        m, k0 = entry
        H, W, B = int(img.shape[-2]), int(img.shape[-1]), int(img.shape[0])
        for name, t, shape in (("mask", m, (H, W)), ("x0", k0, (int(img.shape[1]), H, W))):
            if tuple(t.shape) not in (shape, (B,) + shape) or t.dtype != torch.float32 or t.device != img.device:
                raise _lib.SinddmError(f"keep_maps[{int(s)}] {name} {tuple(t.shape)} {t.dtype} {t.device} does not match the "
                                       f"running sample {tuple(img.shape)} {img.dtype} {img.device} (expected {shape} or "
                                       f"{(B,) + shape} float32)")
        return m.contiguous(), k0.contiguous()

    def _layout_entry(self, s: int, img: torch.Tensor):
        """(layout, N, strength, t_min) of `layout_maps` for scale s, checked against the running sample as `_keep_entry`
        checks its maps, or None (no entry, or strength 0)."""
        if self.layout_maps is None:
            return None
        refuse(self, "layout_maps", "clip")
        lay = self.layout_maps.get(int(s))
        if lay is None:
            return None
        shape = (int(img.shape[1]), int(img.shape[-2]), int(img.shape[-1]))
        bshape = (int(img.shape[0]),) + shape                  # (one picture per sample)
        if shape[0] != 3 or tuple(lay.shape) not in (shape, bshape) or lay.dtype != torch.float32 or lay.device != img.device:
            raise _lib.SinddmError(f"layout_maps[{int(s)}] {tuple(lay.shape)} {lay.dtype} {lay.device} does not match the "
                                   f"running sample {tuple(img.shape)} {img.dtype} {img.device} (expected {shape} or {bshape} "
                                   f"float32)")
        per = lambda v: v.get(int(s), 0) if isinstance(v, dict) else v
        if int(s) not in self.layout_down:
            raise ValueError(f"layout_down has no block size for scale {int(s)}")
        N, g, t_min = int(self.layout_down[int(s)]), float(per(self.layout_strength)), int(per(self.layout_t_min))
        if not 1 <= N <= 64:
            raise ValueError(f"layout_down[{int(s)}] = {N} outside 1 ... 64")
        if not 0.0 <= g <= 1.0 or t_min < 0:
            raise ValueError(f"layout_strength {g} outside [0, 1] or layout_t_min {t_min} < 0 at scale {int(s)}")
        if g == 0.0:
            return None                                        # (the run without the option, resampled or not)
        refuse(self, "layout_maps", "resample")
        return lay.contiguous(), N, g, t_min

    def _layout_gain_for(self, B: int, device) -> Optional[torch.Tensor]:
        """`layout_gain` as B fp32 values on `device`, validated against the running batch, or None."""
        if self.layout_gain is None:
            return None
        g = np.asarray(self.layout_gain.detach().cpu() if isinstance(self.layout_gain, torch.Tensor) else self.layout_gain,
                       dtype=np.float32).reshape(-1)
        if g.shape[0] != int(B):
            raise ValueError(f"layout_gain has {g.shape[0]} values, the batch {int(B)} samples")
        if not bool(np.all((g >= 0.0) & (g <= 1.0))):
            raise ValueError(f"layout_gain {g.tolist()} outside [0, 1]")
        return torch.from_numpy(g.copy()).to(device)

    def _tile_halo(self) -> Tuple[int, int]:
        """(halo_y, halo_x) in pixels of the `tile` setting: _lib.TILE_HALO on a wrapped axis, 0 elsewhere."""
        wy, wx = self.tile
        return (_lib.TILE_HALO if wy else 0, _lib.TILE_HALO if wx else 0)

    @staticmethod
    def _wrap_pad(t: torch.Tensor, hy: int, hx: int) -> torch.Tensor:
        """(..., H, W) -> (..., H + 2 hy, W + 2 hx): the circular pad of the last two axes (sinddm_wrap_halo)."""
        lib = _lib.load()
        t = t.contiguous()
        if t.dtype != torch.float32:
            raise _lib.SinddmError("fp32 only")
        H, W = int(t.shape[-2]), int(t.shape[-1])
        ext = torch.empty(tuple(t.shape[:-2]) + (H + 2 * hy, W + 2 * hx), dtype=t.dtype, device=t.device)
        _lib.check(lib.sinddm_wrap_halo(_lib.ptr(ext), _lib.ptr(t), t.numel() // (H * W), H, W, hy, hx,
                                        _lib.stream_ptr(t.device)), "sinddm_wrap_halo")
        return ext

    def _run_steps(self, img: torch.Tensor, s: int, t_seq) -> torch.Tensor:
        """The reverse steps `t_seq` of scale s (the loop bodies of models.py:477-485,536-546).  Production path: library
        calls that each run many steps (`_ChainCall`) -- the per-step scalars come from a prebuilt table, the states ping-pong
        between two buffers, the N(0,1) draws of models.py:455 are generated inside the step kernel, and Python is not entered
        between steps.  CLIP guidance, intermediate dumps, foreign denoisers, CPU tensors, ROI guidance with
        `chain_guided = False` and `noise_fn` without `chain_noise` go step by step instead (`_p_sample_host_t`, the route
        the parity fixtures pin), which honours every option below through the single-step entries.

        The options of a run, carried by the same call and free to combine except where noted:
          ROI guidance   (every scale but the finest) the edit maps act in the step kernels.
          `tile`         the run works on the sample extended by the wrapped halo -- state, x-tilde, every map and the noise
                         buffers have the extended size -- and returns the centre.  In-kernel draws are keyed on the extended
                         index: a tiled and a plain run of one seed are unrelated.  The step-by-step route extends each
                         network input instead (`_eps`) and steps the centre: the cross-check of the tiled chain.
          `keep_maps`    the scale's mask and known image and the per-step forward scalars: known pixels are replaced inside
                         every step.
          `keep_gated`   the mask is a hold level and every step carries a threshold (functions.gate_thresholds of its landing
                         level and the run's top level): the step keeps the pixels at or above it (sinddm_sample_chain_gate).
                         Same kernels, same launches, same draws and `draw_log` entries as the `keep_maps` run.
          `resample`     (R, J), R > 1: `t_seq` is expanded by functions.resample_schedule; a step that is followed by a jump
                         ends in the step + jump kernel instead of its fused tail.
          `layout_maps`  the steps with t >= layout_t_min run unfused (network, block-delta kernel, layout tail), the others
                         keep their fused tail.  Not with `resample`.
          per sample     a leading batch dimension on a keep / layout map, `roi_bbs_batch`, `layout_gain`: sample b reads
                         slice b.  Neither this nor a layout changes the draws or the `draw_log` entries.
          few steps      `sample_steps` / `sample_spacing`: `t_seq` is thinned by functions.stride_schedule to the levels the
                         network is evaluated at, each step lands on the next of them (`step_coefs_to`); `draw_log` entries
                         keep their shape with those levels as the t list.  `solver_order` = 2: every step runs unfused and
                         ends in the multistep kernel (sinddm_sample_chain_solver).  Not with `resample`; order 2 not with
                         `layout_maps`.
          `keep_window`  with keep maps whose free pixels fit a window smaller than the scale (functions.keep_windows): the
                         run's inputs -- state, x-tilde, mask or hold plane, known image, ROI maps -- are gathered through
                         one window per sample, every map family becomes per-sample, the same steps run on the (B, 3, h, w)
                         tensors on either route, and the result is scattered into the value the full run leaves outside
                         the windows: the kept value of the last step, the known image itself when the run lands on the
                         clean image (`_KeepWindow`).  Not with `tile`, `layout_maps`, CLIP guidance or `noise_fn`.
        The noise is one of five:
          windowed       recorded buffers in pieces of at most CHAIN_NOISE_BYTES, each filled by ONE
                         sinddm_normal_fill_window call at the ids noise_stream_id(s, 'step', pos) of its steps (a second one
                         at the 'jump' ids of its jumps): the draws the full run of `sample_seeds` / `seed_mix` makes at the
                         same absolute positions.  Unseeded: B fresh 62-bit per-sample seeds from torch's CPU generator
                         (unrelated to the unseeded full run of the same torch.manual_seed).  `draw_log`: ("chain_window", s,
                         seeds or (keys, weights), t list, jump targets or None, (h, w), origins).
          `noise_fn` + `chain_noise`   the draws the step-by-step loop would fetch, in its order ('step' per step, 'jump' per
                         jump), handed over as buffers of at most CHAIN_NOISE_BYTES: one call per piece.
          `sample_seeds` sample b's step at position i of the run draws sinddm_normal_fill(3 H W, seed_b,
                         noise_stream_id(s, 'step', i)) in the step kernel; torch's generator is not touched.  `draw_log`:
                         ("chain_seeds", s, seeds, t list), or ("chain_resample", s, seeds, expanded t list, jump targets).
          `seed_mix`     the same with the blend of the row's seeds in place of the one seed's draw
                         (sinddm_sample_chain_mix).  `draw_log`: ("chain_mix", s, (keys, weights), t list, jump targets or None).
          otherwise      one 62-bit seed from torch's CPU generator keys the in-kernel draws.  `draw_log`: ("chain", s, seed,
                         t list), tiled ("chain_tile", ..., (hy, hx)), resampled ("chain_resample", s, seed, ..., jump targets)."""
        plan = RunPlan(self, img, s, t_seq)                    # (every validation and refusal: sampler.RunPlan)
        win = _KeepWindow(self, plan, img) if plan.window is not None else None
        if win is not None:
            plan, img = win.plan, win.img                      # (the same steps on the windows; scattered back by `leave`)
        s, n = plan.s, len(plan.steps)
        fast = ((self.noise_fn is None or self.chain_noise) and isinstance(self.denoise_fn, SinDDMNet)
                and not self.save_interm and not self.clip_guided_sampling and (self.chain_guided or plan.roi is None)
                and n > 0 and img.is_cuda and img.dtype == torch.float32 and img.dim() == 4
                and img.shape[1] == self.channels == 3)
        if not fast:
            hist = torch.empty_like(img) if plan.order2 else None
            for st in plan.steps:
                img = self._p_sample_host_t(img, st.t, s, step_pos=st.pos, q=st.q, hist=hist, plan=plan)
                self._dump_interm(img, s, f'output_t-{st.t:03}_s-{s}.png')
            return img if win is None else win.leave(img)
        run = _ChainCall(self, plan, img)
        x, (kind, src) = run.x, plan.noise
        per, seed, kw = n, 0, {}                               # in-kernel draws: one call for the whole run
        if kind in ("recorded", "window"):
            # pieces of as many steps as fit the byte budget; each piece's draws are fetched exactly as the step-by-step loop
            # fetches them (one `_draw("step", ...)` per step, t = 0 included, in step order, a `_draw("jump", ...)` after a
            # step that jumps) and the next piece continues from the buffer the previous one ended in
            per = max(1, int(CHAIN_NOISE_BYTES) // (x.numel() * x.element_size()))
        elif kind == "seeds":
            kw = dict(sid0=noise_stream_id(s, "step", 0), seeds_dev=torch.tensor(src, dtype=torch.int64, device=x.device))
        elif kind == "mix":
            kw = dict(sid0=noise_stream_id(s, "step", 0), mix_dev=self._mix_tensors(src, x.device))
        else:
            # the step noise is keyed on a 62-bit seed drawn from torch's CPU generator: torch.manual_seed() reproduces a
            # sample, seeding only the CUDA generator (torch.cuda.manual_seed) does not
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
        if kind != "recorded" and self.draw_log is not None:
            self.draw_log.append(plan.log_entry(seed))         # (the draws an entry stands for: RunPlan.log_entry)
        for i0 in range(0, n, per):
            piece = plan.steps[i0:i0 + per]
            if kind == "window":
                # the draws of exactly these steps, each one library call: the steps' slots, then the slots of the jumps
                jumps = [noise_stream_id(s, "jump", st.pos) for st in piece if st.jump is not None]
                kw = dict(noise=win.fill([noise_stream_id(s, "step", st.pos) for st in piece]),
                          jump_noise=(win.fill(jumps) if jumps else torch.empty((1,) + tuple(x.shape), dtype=x.dtype, device=x.device))
                          if plan.jump_to is not None else None)
            if kind == "recorded":
                # (tiled: the draws have the sample's own size and fill the centre of their slot; the halo of a slot is
                # never used -- the halo of a step's output is overwritten with its wrapped centre)
                buf = lambda m: (torch.zeros if run.tiled else torch.empty)((m,) + tuple(x.shape), dtype=x.dtype, device=x.device)
                jn = buf(max(1, sum(st.jump is not None for st in piece))) if plan.jump_to is not None else None
                kw = dict(noise=buf(len(piece)), jump_noise=jn)
                jslots = iter(jn) if jn is not None else None  # (a piece's jumps: one slot each in order of occurrence)
                for st, slot in zip(piece, kw["noise"]):
                    run.centre(slot).copy_(self._draw("step", img.shape, s, st.t, x.device))
                    if st.jump is not None:
                        run.centre(next(jslots)).copy_(self._draw("jump", img.shape, s, st.t, x.device))
            run.call(i0, len(piece), seed, **kw)
        return run.result() if win is None else win.leave(run.result())

    def _eps(self, x, t_dev, t_host, s):
        hy, hx = self._tile_halo()
        if hy or hx:
            # tileable sampling, step by step: the zero-padded network on the input extended by its wrapped halo equals,
            # on the centre, the circularly padded network (the halo is the receptive radius)
            Hc, Wc = int(x.shape[-2]), int(x.shape[-1])
            return self._eps_plain(self._wrap_pad(x, hy, hx), t_dev, t_host, s)[:, :, hy:hy + Hc, hx:hx + Wc].contiguous()
        return self._eps_plain(x, t_dev, t_host, s)

    def _eps_plain(self, x, t_dev, t_host, s):
        if isinstance(self.denoise_fn, SinDDMNet):
            return self.denoise_fn.infer(x, None if t_dev is None else t_dev, int(t_host), float(s))
        if t_dev is None:
            t_dev = torch.full((x.shape[0],), int(t_host), device=x.device, dtype=torch.long)
        return self.denoise_fn(x, t_dev, scale=s)                           # plug point, models.py:356

    def _p_sample_host_t(self, x: torch.Tensor, t: int, s: int, clip_denoised: bool = True, repeat_noise: bool = False,
                         step_pos: int = 0, jump_to: Optional[int] = None, land: Optional[int] = None, q: Optional[float] = None,
                         hist: Optional[torch.Tensor] = None, plan: Optional[RunPlan] = None,
                         t_top: Optional[int] = None) -> torch.Tensor:
        """One reverse step with the timestep known on the host: net forward + ONE fused kernel.  `step_pos`: the step's
        position in its run -- with `sample_seeds` it selects the draw (noise_stream_id(s, 'step', step_pos)).  `jump_to`:
        the level a resampling jump takes the step's output back up to (sinddm_reverse_step_jump: step + jump in one kernel,
        a second draw of kind 'jump'), or None.  `land`: the level the step lands on (None: t - 1; `step_coefs_to`).  `q` /
        `hist`: the multistep factor of the step and the buffer that carries the previous step's clean estimate
        (sinddm_reverse_step_ms: `hist` is written, and read when q != 0), or None.  `t_top`: the highest level of the run the
        step belongs to -- with `keep_gated` it sets the step's threshold (functions.gate_thresholds).  `plan`: the run's plan when `_run_steps`
        steps through it -- the step is its record `step_pos`; else the one-step plan of the arguments is built here."""
        if (q is None) != (hist is None):
            raise ValueError("a multistep step takes q and hist together")
        if plan is None:
            plan, step_pos = RunPlan(self, x, s, [t], at=(step_pos, jump_to, land, q, t_top), clip_denoised=clip_denoised), 0
        st = plan.steps[step_pos]
        if self.clip_guided_sampling:
            if self.clip_model is None or self.guidance_sub_iters is None or self.stop_guidance is None:
                raise RuntimeError("clip_guided_sampling is set but clip_model / guidance_sub_iters / stop_guidance are not: "
                                   "CLIP is outside this build -- assign any object with zero_grad() and a differentiable "
                                   "calculate_clip_loss(image, text_embedds) (reference models.py:193-220, 367-421)")
            return self._p_sample_guided(x.contiguous(), st.t, int(s), clip_denoised, repeat_noise, st.pos)
        x = x.contiguous()
        eps = self._eps(x, None, st.t, s)
        if self.save_interm:                                                # models.py:360-366 (x_recon lives inside the fused kernel:
            tt = torch.full((x.shape[0],), st.t, device=x.device, dtype=torch.long)     # recomputed here, for the dump only)
            self._dump_x_recon(self.predict_start_from_noise(x, t=tt, s=s, noise=eps)[0], st.t, s)
        # (a windowed run's draws are the full run's at the window's absolute positions: `_KeepWindow.draw`)
        draw = plan.win.draw if plan.win is not None else (lambda kind, st: self._draw(kind, x.shape, s, st.t, x.device, st.pos))
        z = noise_like(x.shape, x.device, True).contiguous() if repeat_noise else draw("step", st)
        z2 = draw("jump", st) if st.jump is not None else None
        out = torch.empty_like(x)
        if plan.per[0] or plan.per[1] or plan.per[2] or (st.g > 0.0 and (plan.per[3] or plan.gain is not None)):
            # per-sample maps: the single-step entries with B = 1 on each sample's slices (a cross-check route)
            for b in range(x.shape[0]):
                self._step_tail(plan, st, x, eps, z, z2, out, hist, b)
        else:
            self._step_tail(plan, st, x, eps, z, z2, out, hist)
        return out

    def _step_tail(self, plan, st, x, eps, z, z2, out, hist, b=None):
        """The single-step entry that ends the step `st` of `plan` on the route of `_p_sample_host_t`: `out` is written.  The
        first that applies: a layout pull (st.g > 0), a resampling jump (second draw z2), a multistep step (`hist`), keep maps,
        ROI maps, the plain step.  `b`: sample b alone -- slice b of every tensor, row b of every per-sample map (B = 1).
        A gated step (st.thr) ends in sinddm_reverse_step_keep_gate; the pull, jump and multistep entries take no threshold
        and get the step's own mask (hold level >= st.thr) as 0 / 1, which is what the gate hands the chain's kernels."""
        lib, xt, g = _lib.load(), plan.xt, st.g
        ew, ec = plan.roi if plan.roi is not None else (None, None)
        km, kx = plan.keep if plan.keep is not None else (None, None)
        lay, N = plan.lay[:2] if st.g > 0.0 else (None, 0)
        if b is not None:
            x, eps, xt, z, z2, out, hist = (None if v is None else v[b:b + 1] for v in (x, eps, xt, z, z2, out, hist))
            row = lambda v, nd: v if v is None or v.dim() == nd else v[b]
            ew, km, ec, kx, lay = row(ew, 2), row(km, 2), row(ec, 3), row(kx, 3), row(lay, 3)
            if plan.gain is not None:                          # (the strength the chain's kernel forms: the fp32 product)
                g = float(np.float32(g) * plan.gain[b])
        gate_entry = st.thr is not None and lay is None and st.jump is None and hist is None
        if st.thr is not None and not gate_entry:
            km = (km >= st.thr).to(km.dtype).contiguous()      # (an fp32 compare: st.thr is an fp32 value)
        B_, C_, H_, W_ = x.shape
        head = [_lib.ptr(v) for v in (x, eps, xt, z, out)] + [C.byref(st.k)]
        maps = [_lib.ptr(ew), _lib.ptr(ec), _lib.ptr(km), _lib.ptr(kx), *st.ab]
        shp = [B_, C_, H_ * W_, _lib.stream_ptr(x.device)]
        if lay is not None:
            # the conditioned step: block deltas of (layout - x_recon), then the step with c_eff = ec + g * U(D)
            delta = torch.empty(B_ * 3 * (-(-H_ // N)) * (-(-W_ // N)), dtype=x.dtype, device=x.device)
            _lib.check(lib.sinddm_layout_delta(*head[:3], _lib.ptr(lay), _lib.ptr(delta), head[5], *maps[:2], N, B_, H_, W_, 0, 0,
                                               shp[3]), "sinddm_layout_delta")
            name, args = "sinddm_reverse_step_layout", [*head, _lib.ptr(delta), g, N, *maps, B_, H_, W_, 0, 0,
                                                        int(bool(self.tile[0])), int(bool(self.tile[1])), shp[3]]
        elif st.jump is not None:
            name, args = "sinddm_reverse_step_jump", [*head[:4], _lib.ptr(z2), *head[4:], C.byref(st.jump), *maps, *shp]
        elif hist is not None:
            name, args = "sinddm_reverse_step_ms", [*head, st.q, _lib.ptr(hist), *maps, *shp]
        elif gate_entry:
            name, args = "sinddm_reverse_step_keep_gate", [*head, *maps, *shp, st.thr]
        elif km is not None:
            name, args = "sinddm_reverse_step_keep", [*head, *maps, *shp]
        elif ew is not None:
            name, args = "sinddm_reverse_step_edit", [*head, *maps[:2], *shp]
        else:
            name, args = "sinddm_reverse_step", [*head, x.numel(), shp[3]]
        _lib.check(getattr(lib, name)(*args), name)

    @torch.no_grad()
    def p_sample(self, x, t, s, clip_denoised=True, repeat_noise=False):   # models.py:449-459
        t_host = int(t[0]) if isinstance(t, torch.Tensor) else int(t)      # the reference also reads t[0] (:331,:434)
        return self._p_sample_host_t(x, t_host, int(s), clip_denoised, repeat_noise)

    @torch.no_grad()
    def p_sample_loop(self, shape, s):                                     # models.py:462-487
        device = self.betas.device
        img = self._draw("init", shape, s, 0, device)
        self._dump_interm(img, s, f'input_noise_s-{s}.png')
        t_min = self.num_timesteps_ideal[s + 1] if self.sample_limited_t and s < (self.n_scales - 1) else 0
        return self._run_steps(img, s, reversed(range(t_min, self.num_timesteps)))

    def _dump_interm(self, img, s, name, renorm=True):
        """save_interm=True (models.py:469-485,520-546): PNG grid of the running sample after every step (debug aid)."""
        if not self.save_interm:
            return
        from .trainer import save_image
        folder = Path(str(self.results_folder / f'interm_samples_scale_{s}'))
        folder.mkdir(parents=True, exist_ok=True)
        save_image((img + 1) * 0.5 if renorm else img, str(folder / name), nrow=4)

    def _dump_x_recon(self, x_recon, t_host: int, s: int):
        """save_interm=True: the denoised estimate of the step, `denoised_t-TTT_s-S.png` (models.py:360-366)."""
        self._dump_interm(x_recon.clamp(-1., 1.), s, f'denoised_t-{int(t_host):03}_s-{int(s)}.png')

    @torch.no_grad()
    def sample(self, batch_size=16, scale_0_size=None, s=0):               # models.py:489-499
        image_size = scale_0_size if scale_0_size is not None else self.image_sizes[0]
        return self.p_sample_loop((batch_size, self.channels, image_size[0], image_size[1]), s=s)

    @torch.no_grad()
    def p_sample_via_scale_loop(self, batch_size, img, s, custom_t=None):  # models.py:501-547
        total_t = int(self.num_timesteps_ideal[min(s, self.n_scales - 1)] - 1 if custom_t is None else custom_t)
        self.img_prev_upsample = img                                        # x-tilde of this scale
        noise = self._draw("renoise", img.shape, s, 0, img.device)
        img = self._q_sample_impl(img, None, total_t, noise)                # models.py:518
        self._dump_interm(img, s, f'noisy_input_s_{s}.png')
        if self.clip_mask is not None:                                      # models.py:528-535
            if s > 0:
                mul_size = [int(self.image_sizes[s][0] * self.scale_mul[0]), int(self.image_sizes[s][1] * self.scale_mul[1])]
                self.clip_mask = F.interpolate(self.clip_mask, size=mul_size, mode='bilinear')
                self.x_recon_prev = F.interpolate(self.x_recon_prev, size=mul_size, mode='bilinear')
            else:                                                           # a mask created at scale 0 is too noisy
                self.clip_mask = None
        t_min = self.num_timesteps_ideal[s + 1] if self.sample_limited_t and s < (self.n_scales - 1) else 0
        return self._run_steps(img, s, reversed(range(t_min, total_t)))

    def target_size(self, s, scale_mul=(1, 1), custom_sample=False, custom_img_size_idx=0, custom_image_size=None):
        """Size selection of sample_via_scale (models.py:554-565), int() truncation included."""
        if custom_sample:
            if custom_img_size_idx >= self.n_scales:
                size = self.image_sizes[self.n_scales - 1]
                factor = self.scale_factor ** (custom_img_size_idx + 1 - self.n_scales)
                size = (int(size[0] * factor), int(size[1] * factor))
            else:
                size = self.image_sizes[custom_img_size_idx]
        else:
            size = self.image_sizes[s]
        image_size = (int(size[0] * scale_mul[0]), int(size[1] * scale_mul[1]))
        if custom_image_size is not None:
            image_size = custom_image_size
        return image_size

    def upsample(self, img: torch.Tensor, size) -> torch.Tensor:
        """F.interpolate(img, size, mode='bilinear') on the HIP kernel (models.py:567); on an axis `tile` wraps, the
        interpolation of the image's periodic continuation (sinddm_upsample_bilinear_wrap)."""
        lib = _lib.load()
        img = img.contiguous()
        B, Cc, h, w = img.shape
        H, W = int(size[0]), int(size[1])
        out = torch.empty((B, Cc, H, W), dtype=img.dtype, device=img.device)
        if any(self.tile):
            _lib.check(lib.sinddm_upsample_bilinear_wrap(_lib.ptr(img), _lib.ptr(out), B * Cc, h, w, H, W,
                                                         int(bool(self.tile[0])), int(bool(self.tile[1])),
                                                         _lib.stream_ptr(img.device)), "sinddm_upsample_bilinear_wrap")
            return out
        _lib.check(lib.sinddm_upsample_bilinear(_lib.ptr(img), _lib.ptr(out), B * Cc, h, w, H, W,
                                                _lib.stream_ptr(img.device)), "sinddm_upsample_bilinear")
        return out

    @torch.no_grad()
    def sample_via_scale(self, batch_size, img, s, scale_mul=(1, 1), custom_sample=False, custom_img_size_idx=0,
                         custom_t=None, custom_image_size=None):           # models.py:549-568
        image_size = self.target_size(s, scale_mul, custom_sample, custom_img_size_idx, custom_image_size)
        img = self.upsample(img, image_size)
        return self.p_sample_via_scale_loop(batch_size, img, s, custom_t=custom_t)

    def _q_sample_impl(self, x0, t_dev, t_host, noise, x_orig=None, gamma_row=None, halo=(0, 0), crop=None, windows=None):
        """x_t of q_sample / the gamma-mixed x_noisy of p_losses (sinddm_q_sample); with a `halo` = (hy, hx) the same, written
        extended by its wrapped halo in one pass (sinddm_q_sample_wrap): (B,C,H + 2 hy,W + 2 hx); with a `crop` = (h, w) and
        the int32 (B,2) device table `windows`, read through one window per sample (sinddm_q_sample_crop): `noise` and the
        result are (B,C,h,w)."""
        lib = _lib.load()
        x0 = x0.contiguous()
        noise = noise.contiguous()
        if t_dev is not None:
            t_dev = t_dev.to(device=x0.device, dtype=torch.int64).contiguous()
        if crop is not None:
            B, Cc, H, W = x0.shape
            h, w = crop
            if tuple(noise.shape) != (B, Cc, h, w):
                raise _lib.SinddmError(f"q_sample: noise {tuple(noise.shape)} is not the window batch {(B, Cc, h, w)}")
            out = torch.empty_like(noise)
            _lib.check(lib.sinddm_q_sample_crop(_lib.ptr(x0), _lib.ptr(x_orig.contiguous()) if x_orig is not None else None,
                                                _lib.ptr(noise), _lib.ptr(out), _lib.ptr(self.sqrt_alphas_cumprod),
                                                _lib.ptr(self.sqrt_one_minus_alphas_cumprod),
                                                _lib.ptr(gamma_row) if gamma_row is not None else None,
                                                _lib.ptr(t_dev) if t_dev is not None else None, int(t_host),
                                                _lib.ptr(windows), B, Cc, H, W, h, w, _lib.stream_ptr(x0.device)),
                       "sinddm_q_sample_crop")
            return out
        hy, hx = halo
        if hy or hx:
            B, Cc, H, W = x0.shape
            out = torch.empty((B, Cc, H + 2 * hy, W + 2 * hx), dtype=x0.dtype, device=x0.device)
            _lib.check(lib.sinddm_q_sample_wrap(_lib.ptr(x0), _lib.ptr(x_orig.contiguous()) if x_orig is not None else None,
                                                _lib.ptr(noise), _lib.ptr(out), _lib.ptr(self.sqrt_alphas_cumprod),
                                                _lib.ptr(self.sqrt_one_minus_alphas_cumprod),
                                                _lib.ptr(gamma_row) if gamma_row is not None else None, _lib.ptr(t_dev),
                                                int(t_host), B, Cc, H, W, hy, hx, _lib.stream_ptr(x0.device)),
                       "sinddm_q_sample_wrap")
            return out
        out = torch.empty_like(x0)
        B = x0.shape[0]
        n = x0.numel() // B
        _lib.check(lib.sinddm_q_sample(_lib.ptr(x0), _lib.ptr(x_orig.contiguous()) if x_orig is not None else None,
                                       _lib.ptr(noise), _lib.ptr(out), _lib.ptr(self.sqrt_alphas_cumprod),
                                       _lib.ptr(self.sqrt_one_minus_alphas_cumprod),
                                       _lib.ptr(gamma_row) if gamma_row is not None else None,
                                       _lib.ptr(t_dev) if t_dev is not None else None, int(t_host), B, n,
                                       _lib.stream_ptr(x0.device)), "sinddm_q_sample")
        return out

    def q_sample(self, x_start, t, noise=None):                            # models.py:570-576
        noise = default(noise, lambda: torch.randn_like(x_start))
        return self._q_sample_impl(x_start, t, 0, noise)

    def _draw_windows(self, s, shape):
        """The (B,2) window origins of a cropped step at scale s: `crop_fn`, else the clamped draw (functions.crop_windows) from
        the private generator -- a host draw, no device sync; under data parallelism every rank draws its own."""
        B, _, H, W = shape
        if self.crop_fn is not None:
            return self.crop_fn(self.crop_step, int(s), int(B))
        if self._crop_gen is None:
            from . import dist as sdist
            self._crop_gen = torch.Generator()
            self._crop_gen.manual_seed(sdist.seed_for_rank(torch.initial_seed() % (2 ** 62)))
        return crop_windows(self._crop_gen, B, (H, W), self.train_crop, self.train_crop_margin)

    def p_losses(self, x_start, t, s, noise=None, x_orig=None, windows=None):   # models.py:578-611
        """The loss of one training step, as `train_step.TrainStep` describes it (every check runs there, before any launch).
        With `train_tile` (no reference line: padding_mode='circular' on the reference's nn.Conv2d's while it trains) x_noisy is
        written extended by its wrapped halo, the zero-padded training forward runs on the extended image and the loss is
        taken on the centre: the gradient handed back is 0 on the halo, and every parameter gradient equals the circularly
        padded network's.  With `train_weights` the loss is sum(w e) / (B C sum w) instead of the mean.  With
        `train_crop`, at a scale larger than the crop, x_noisy is one window per sample (`windows`: (B,2) origins, else
        `crop_fn`, else the clamped draw), `noise` has the window's size, and the loss is
        sum_b sum_c sum_{p in V_b} w(p) e / (C sum_b sum_{p in V_b} w(p)) over the valid rectangles V_b."""
        plan = TrainStep(self, x_start.shape, s, windows=windows, draw=lambda: self._draw_windows(s, x_start.shape))
        x_orig = x_orig if plan.s > 0 else None
        if plan.crop is not None:
            win, rects = plan.tables(x_start.device)
            noise = default(noise, lambda: torch.randn(plan.ext_shape, dtype=x_start.dtype, device=x_start.device))
            x_noisy = self._q_sample_impl(x_start, t, 0, noise, x_orig=x_orig, gamma_row=plan.gamma_row, crop=plan.crop,
                                          windows=win)
            x_recon = self.denoise_fn(x_noisy, t, plan.s)                   # (window size, like x_noisy)
            return self._step_loss(plan, noise, x_recon, x_start, x_orig, t, win, rects)
        noise = default(noise, lambda: torch.randn_like(x_start))
        x_noisy = self._q_sample_impl(x_start, t, 0, noise, x_orig=x_orig, gamma_row=plan.gamma_row, halo=plan.halo)
        x_recon = self.denoise_fn(x_noisy, t, plan.s)                       # (extended by the halo, like x_noisy)
        return self._step_loss(plan, noise, x_recon, x_start, x_orig, t)

    def _step_loss(self, plan, noise, x_recon, x_start, x_orig, t, win=None, rects=None):
        """The loss of the step `plan` on the network's output `x_recon` (extended by the plan's halo, or of the plan's crop:
        `win` / `rects` are then the plan's tables on the device)."""
        if plan.crop is not None:
            if plan.loss_type == 'l1':
                return l1_loss(noise, x_recon, (0, 0), plan.weight, plan.inv_norm, win, rects)
            # 'l2' and 'l1_pred_img' as below: torch ops, on a per-sample (B,1,h,w) weight built from the tables on the device
            (B, _, _, _), (h, w) = plan.shape, plan.crop
            ys = torch.arange(h, device=win.device)[None, :, None]
            xs = torch.arange(w, device=win.device)[None, None, :]
            r = rects.long()
            wb = ((ys >= r[:, 0, None, None]) & (ys < r[:, 1, None, None]) & (xs >= r[:, 2, None, None])
                  & (xs < r[:, 3, None, None])).to(x_recon.dtype)
            gy, gx = win[:, 0, None, None].long() + ys, win[:, 1, None, None].long() + xs        # full-image positions
            if plan.weight is not None:
                wb = wb * plan.weight[gy, gx]
            wb = wb[:, None]
            if plan.loss_type == 'l2':
                return ((noise - x_recon) ** 2 * wb).sum() * plan.inv_norm
            target = self._mix_prev(plan, x_start, x_orig, t)
            bi = torch.arange(B, device=win.device)[:, None, None, None]
            ci = torch.arange(target.shape[1], device=win.device)[None, :, None, None]
            target = target[bi, ci, gy[:, None], gx[:, None]]                 # the same windows of the target
            return ((target - x_recon).abs() * wb).sum() * plan.inv_norm
        if plan.loss_type == 'l1':     # what main.py:97 selects: one fused kernel (loss, gradient, the halo's and the holes' zeros)
            return l1_loss(noise, x_recon, plan.halo, plan.weight, plan.inv_norm)
        # the two loss types main.py never selects (models.py:595-607): the network's forward / backward are the HIP path
        # (x_recon carries its autograd node), the loss itself is elementwise torch ops on the centre
        (_, _, H, W), (hy, hx), w = plan.shape, plan.halo, plan.weight
        if hy or hx:
            x_recon = x_recon[:, :, hy:hy + H, hx:hx + W]                   # (its backward zero-fills the halo)
        if plan.loss_type == 'l2':
            return F.mse_loss(noise, x_recon) if w is None else ((noise - x_recon) ** 2 * w).sum() * plan.inv_norm
        x_mix_prev = self._mix_prev(plan, x_start, x_orig, t)
        return (x_mix_prev - x_recon).abs().mean() if w is None else ((x_mix_prev - x_recon).abs() * w).sum() * plan.inv_norm

    def _mix_prev(self, plan, x_start, x_orig, t):
        """The target of 'l1_pred_img' (models.py:597-606): the gamma mix of the level below t."""
        if plan.s == 0:
            return x_start
        if int(t[0]) > 0:                                                   # (the reference's host sync, models.py:599)
            g = extract(plan.gamma_row, t - 1, x_start.shape)
            return g * x_start + (1 - g) * x_orig
        return x_orig

    @torch.no_grad()
    def denoise_score(self, y, s, y_prev=None, levels=None, draws=1, seeds=None, weight=None):
        """What the model finds implausible in `y`, per pixel (no reference counterpart; score.py, sinddm_score_chain): the
        training L1 loss  |z - eps(x_t, t, s)|  of the (B,3,H,W) batch `y` at scale `s`, evaluated with the inference network
        at every level of `levels` (default: score.score_levels(num_timesteps_trained[s], 10); each validated against the
        levels the scale was trained on) over `draws` noise draws.  `y_prev` is the blurred image of the scale -- the scale
        below upsampled, training's x_recon -- required at s > 0 and refused at s == 0.  Returns (map, table):
            map    (B,H,W)        the mean of |z - eps| over levels, draws and channels, times `weight`; under a weight it
                                  is divided by nothing else: holes are exactly 0
            table  (n_levels,B)   per level, the mean over draws, channels and pixels -- over sum(weight) under a weight
        `weight`: an (H,W) float32 plane on y's device, finite and >= 0, shared by the batch (the hard train mask: a masked
        model is not scored against its hole).  The draws are folded into the batch: row b * draws + r is sample b under its
        r-th draw, so coarse scales fill the GPU, and one library call (per 1024 levels) does the rest on the current stream.
        `seeds`: None (one key from torch's CPU generator for the call) or B * draws ints in [0, 2^63), row-major as above: a
        row's draws then depend on its seed alone, and its map on nothing else up to fp32 rounding (the kernels a batch
        takes, and above 2^23 quads per call the rounding of x_t, may change with the batch size: include/sinddm_hip.h).
        A weight that is not finite, negative somewhere or zero everywhere is refused.
        Stream ids: score.score_stream_id(s, position in `levels`).
        `tile` on any axis: NotImplementedError (the wrapped-halo score is not built)."""
        from .score import check_score_args, score_stream_id
        y = torch.as_tensor(y)
        s, levels, draws, seeds = check_score_args(self, y, s, y_prev, levels, draws, seeds, weight)
        lib, net = _lib.load(), self.denoise_fn
        B, _, H, W = (int(v) for v in y.shape)
        R = B * draws
        rep = (lambda t: t.repeat_interleave(draws, dim=0).contiguous()) if draws > 1 else (lambda t: t.contiguous())
        yr = rep(y)
        pr = rep(y_prev) if y_prev is not None else None
        x_t = torch.empty_like(yr)
        smap = torch.empty((R, H, W), dtype=torch.float32, device=y.device)
        if seeds is not None:
            key, seeds_dev = 0, torch.tensor(seeds, dtype=torch.int64, device=y.device)
        else:
            key, seeds_dev = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)), None
        wt = weight.contiguous() if weight is not None else None
        opts = _lib.ScoreOpts(_lib.ptr(wt), _lib.ptr(seeds_dev))
        gamma_row = self.gammas[s - 1].contiguous() if s > 0 else None
        packed = net.packed_weights()
        total = torch.zeros((R, H, W), dtype=torch.float32, device=y.device) if len(levels) > _lib.SCORE_MAX_EVALS else None
        tables = []
        for i0 in range(0, len(levels), _lib.SCORE_MAX_EVALS):
            piece = levels[i0:i0 + _lib.SCORE_MAX_EVALS]
            n = len(piece)
            ws = _workspace(y.device, lib.sinddm_score_workspace_bytes(net.dim_arg, R, H, W, n))
            lev = torch.empty((n, R), dtype=torch.float32, device=y.device)
            tl = (C.c_int * n)(*piece)
            _lib.check(lib.sinddm_score_chain(_lib.ptr(net.flat_params), _lib.ptr(packed), _lib.ptr(yr), _lib.ptr(pr),
                                              _lib.ptr(x_t), _lib.ptr(self.sqrt_alphas_cumprod),
                                              _lib.ptr(self.sqrt_one_minus_alphas_cumprod), _lib.ptr(gamma_row), tl, n, float(s),
                                              key, score_stream_id(s, i0), _lib.ptr(smap), _lib.ptr(lev), net.dim_arg, R, H, W,
                                              ws.data_ptr(), ws.numel(), _lib.stream_ptr(y.device), C.byref(opts)),
                       "sinddm_score_chain")
            tables.append(lev)
            if total is not None:
                total += smap
        if total is not None:
            smap = total
        norm = float(weight.double().sum()) if weight is not None else float(H * W)
        table = torch.cat(tables).view(len(levels), B, draws).mean(dim=2) / (3.0 * norm)
        smap = smap.view(B, draws, H, W).mean(dim=1) / (3.0 * len(levels))
        return smap, table

    def forward(self, x, s, *args, **kwargs):                              # models.py:613-631
        s = int(s)
        img = x[0]
        x_orig = x[0] if s > 0 else None
        x_start = x[1] if s > 0 else x[0]
        b, c, h, w = img.shape
        img_size = self.image_sizes[s]
        assert h == img_size[0] and w == img_size[1], f'height and width of image must be {img_size}'
        t = torch.randint(0, self.num_timesteps_trained[s], (b,), device=img.device).long()
        return self.p_losses(x_start, t, s, *args, x_orig=x_orig, **kwargs)
