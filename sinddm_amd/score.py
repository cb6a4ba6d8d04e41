"""Denoising-score maps: the host side (plain Python) of `MultiScaleGaussianDiffusion.denoise_score` and
`MultiscaleTrainer.score`.  The quantity is the per-pixel term of the training loss,  E_{t,z} |z - eps_theta(x_t, t, s)|,
evaluated on any picture by sinddm_score_chain (include/sinddm_hip.h): what the model finds implausible, per pixel.

    score_levels      which noise levels a score averages over
    score_stream_id   the Philox stream of evaluation i of a scale (the ONE owner of that layout)
    score_pyramid     a picture brought to every scale, with each scale's blurred partner
    score_edit_map    a score map normalised against the training image's own: a strength map for `--mode edit`
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

# Stream ids of the score draws: (s << 32) | (SCORE_STREAM + i) for evaluation i at scale s.  The sampler's ids of a scale
# are k = 0, 1, 2 + i and 2^31 + 2 + i (models.noise_stream_id): with i below 2^30 - 2 a step stays under 2^30, and a jump's
# second draw starts at 2^31; the score's range [2^30, 2^31) lies between the two and meets neither.
SCORE_STREAM = 0x40000000
SCORE_STREAM_END = 0x80000000


def score_stream_id(s: int, i: int = 0) -> int:
    """Stream id of evaluation i of a score at scale s."""
    s, i = int(s), int(i)
    if not 0 <= s < (1 << 31) or not 0 <= i < SCORE_STREAM_END - SCORE_STREAM:
        raise ValueError(f"score_stream_id: scale {s} / evaluation {i} out of range")
    return (s << 32) | (SCORE_STREAM + i)


def score_levels(T: int, n: int) -> List[int]:
    """`n` noise levels spread over 0 ... T - 1, both ends included, strictly increasing; n > T gives every level.  n == 1
    gives the middle level."""
    T, n = int(T), int(n)
    if T < 1 or n < 1:
        raise ValueError(f"score_levels: T = {T} and n = {n} must be >= 1")
    n = min(n, T)
    if n == 1:
        return [(T - 1) // 2]
    # (integer arithmetic: round-half-up of i (T - 1) / (n - 1); the spacing is >= 1, so the levels are distinct)
    return [(2 * i * (T - 1) + (n - 1)) // (2 * (n - 1)) for i in range(n)]


def score_pyramid(img, sizes, upsample=None) -> List[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    """A (3, H, W) picture (or a (N, 3, H, W) stack) at the finest size brought to every (h, w) of `sizes`: a list of
    (y, y_prev) per scale, both (N, 3, h, w) fp32 on the picture's device.  y is the area average of the picture
    (functions._layout_pyramid); y_prev, at a scale > 0, is the scale below upsampled bilinearly to (h, w) -- `upsample(t,
    (h, w))`, by default sinddm_upsample_bilinear (`MultiScaleGaussianDiffusion.upsample`'s kernel) -- and None at scale 0.
    That is how training's blurred partner is made from the scale below, but not from the same FILES: the training image
    itself is scored from its own `data_list` pair, the pictures the weights were trained on (MultiscaleTrainer.score)."""
    from .functions import _layout_pyramid
    pic = torch.as_tensor(img)
    if pic.dim() == 3:
        pic = pic[None]
    if pic.dim() != 4 or pic.shape[1] != 3 or pic.shape[0] < 1:
        raise ValueError(f"score_pyramid: the picture must be (3, H, W) or (N, 3, H, W), got {tuple(pic.shape)}")
    sizes = [(int(h), int(w)) for h, w in sizes]
    if tuple(pic.shape[2:]) != sizes[-1]:
        raise ValueError(f"score_pyramid: the picture {tuple(pic.shape[2:])} is not the finest size {sizes[-1]}")
    ys = [y.to(torch.float32).contiguous() for y in _layout_pyramid(pic.to(torch.float32), sizes)]
    if upsample is None:
        upsample = _upsample_bilinear
    out = []
    for s, y in enumerate(ys):
        out.append((y, None if s == 0 else upsample(ys[s - 1], sizes[s]).contiguous()))
    return out


def _upsample_bilinear(t: torch.Tensor, size) -> torch.Tensor:
    from . import _lib
    lib = _lib.load()
    t = t.contiguous()
    B, Cc, h, w = t.shape
    out = torch.empty((B, Cc, int(size[0]), int(size[1])), dtype=t.dtype, device=t.device)
    _lib.check(lib.sinddm_upsample_bilinear(_lib.ptr(t), _lib.ptr(out), B * Cc, h, w, int(size[0]), int(size[1]),
                                            _lib.stream_ptr(t.device)), "sinddm_upsample_bilinear")
    return out


def score_edit_map(S_img, S_train, valid=None) -> torch.Tensor:
    """clamp((S_img - m) / (M - m), 0, 1) with m the median and M the maximum of the training image's own score map
    `S_train` at that scale: 0 where the picture scores no worse than the typical training pixel, 1 where it scores as badly
    as the training image's worst pixel or worse -- "redraw what the model finds implausible, keep the rest", the strength
    map `--mode edit` takes.  The median is the lower one (torch.median).  A flat S_train (M == m) gives the step S_img > m.
    `valid`: None, or a mask of S_train's shape (non-zero = counts) -- under a weight plane the holes of a score map are exact
    zeros that say nothing about the model, so m and M are taken over the valid pixels only (and the picture's own holes, 0 in
    S_img, come out 0: left alone)."""
    a = torch.as_tensor(S_img).to(torch.float32)
    t = torch.as_tensor(S_train).to(torch.float32)
    if valid is not None:
        v = torch.as_tensor(valid).to(t.device)
        if tuple(v.shape) != tuple(t.shape):
            raise ValueError(f"score_edit_map: valid {tuple(v.shape)} is not the training map {tuple(t.shape)}")
        t = t[v != 0]
    if t.numel() < 1:
        raise ValueError("score_edit_map: the training image's map is empty")
    m, M = t.flatten().median(), t.max()
    if not bool(torch.isfinite(m)) or not bool(torch.isfinite(M)):
        raise ValueError("score_edit_map: the training image's map is not finite")
    if float(M) <= float(m):
        return (a > m).to(torch.float32)
    return ((a - m) / (M - m)).clamp(0.0, 1.0)


def check_score_args(d, y, s, y_prev, levels, draws, seeds, weight):
    """Every check of `denoise_score` that needs no device: returns (s, the levels as a list, draws, the seeds as a list or
    None).  `d` is the diffusion object (its `n_scales`, `num_timesteps_trained`, `tile`)."""
    s = int(s)
    if not 0 <= s < int(d.n_scales):
        raise ValueError(f"denoise_score: scale {s} outside 0 ... {int(d.n_scales) - 1}")
    if any(bool(v) for v in d.tile):
        raise NotImplementedError("denoise_score under `tile`: the score of the wrapped-halo network is not built")
    if y.dim() != 4 or y.shape[1] != 3 or y.shape[0] < 1:
        raise ValueError(f"denoise_score: y must be (B, 3, H, W), got {tuple(y.shape)}")
    if s == 0 and y_prev is not None:
        raise ValueError("denoise_score: scale 0 has no blurred image (y_prev must be None)")
    if s > 0 and y_prev is None:
        raise ValueError(f"denoise_score: scale {s} needs y_prev, the scale below upsampled (training's x_recon)")
    if y_prev is not None and (tuple(y_prev.shape) != tuple(y.shape) or y_prev.dtype != y.dtype or y_prev.device != y.device):
        raise ValueError(f"denoise_score: y_prev {tuple(y_prev.shape)} {y_prev.dtype} {y_prev.device} does not match y "
                         f"{tuple(y.shape)} {y.dtype} {y.device}")
    if y.dtype != torch.float32:
        raise ValueError(f"denoise_score: y must be float32, got {y.dtype}")
    T = int(d.num_timesteps_trained[s])
    levels = score_levels(T, 10) if levels is None else [int(t) for t in levels]
    if not levels:
        raise ValueError("denoise_score: no levels")
    for t in levels:
        if not 0 <= t < T:
            raise ValueError(f"denoise_score: level {t} outside 0 ... {T - 1}, the levels scale {s} was trained on")
    draws = int(draws)
    if draws < 1:
        raise ValueError(f"denoise_score: draws = {draws} must be >= 1")
    B = int(y.shape[0])
    if seeds is not None:
        seeds = [int(v) for v in seeds]
        if len(seeds) != B * draws:
            raise ValueError(f"denoise_score: {len(seeds)} seeds for {B} samples x {draws} draws")
        if min(seeds) < 0 or max(seeds) >= (1 << 63):
            raise ValueError("denoise_score: a seed must be in [0, 2^63)")
    if weight is not None:
        if tuple(weight.shape) != tuple(y.shape[2:]):
            raise ValueError(f"denoise_score: weight {tuple(weight.shape)} is not the image plane {tuple(y.shape[2:])}")
        if weight.dtype != torch.float32 or weight.device != y.device:
            raise ValueError("denoise_score: weight must be float32 on y's device")
        if not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
            raise ValueError("denoise_score: weight must be finite and >= 0")
        if not bool((weight > 0).any()):
            raise ValueError("denoise_score: the weight plane is zero everywhere: nothing to score, and no mean over sum(w)")
    return s, levels, draws, seeds
