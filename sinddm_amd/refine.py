"""Acting on the patch nearest-neighbour field: the patch vote, and the refinement loop built from field and vote.

`metrics.patch_nnf` says which patch of the training image every patch of a sample is nearest to; `patch_vote` replaces
every patch by that one and makes every pixel the mean of the patches that cover it (`sinddm_patch_vote`,
csrc/patch_vote.h; the contract is in include/sinddm_hip.h).  Field then vote is the EM step of GPNN ("Drop the GAN"):
coordinate descent on the patch energy E(x) = sum_i min_j |P_i x - b_j|^2, so with blend = 1 and the plain field the
energy cannot rise.  `patch_refine` iterates it, optionally with GPNN's completeness normalisation (`alpha`): the search
then ranks by D_ij / (alpha 3 P^2 + min_i D_ij) (`sinddm_patch_nnf_scaled`), which pulls the sample towards showing every
patch of the image.  There is no CPU route.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import SinddmError
from .metrics import PATCHES, _wrap_bits, grid_size, patch_nnf


def check_blend(blend, what="patch_vote") -> float:
    try:
        b = float(blend)
    except (TypeError, ValueError):
        raise SinddmError(f"{what}: blend must be a number in [0, 1], got {blend!r}") from None
    if not math.isfinite(b) or not 0.0 <= b <= 1.0:
        raise SinddmError(f"{what}: blend must be in [0, 1], got {blend!r}")
    return b


@dataclass
class PatchRefine:
    """The `patch_refine` option of `MultiscaleTrainer.sample_scales`: `iters` field-and-vote iterations with patch size
    `patch` after the chain of every scale in `scales` = (a, b), inclusive (None: every scale); `alpha` and `blend` as
    `patch_refine` takes them."""
    iters: int = 1
    patch: int = 7
    alpha: Optional[float] = None
    blend: float = 1.0
    scales: Optional[Tuple[int, int]] = None

    @classmethod
    def of(cls, opt) -> "PatchRefine":
        """A `PatchRefine`, or a dict of its fields, checked."""
        if isinstance(opt, dict):
            unknown = set(opt) - set(cls.__dataclass_fields__)
            if unknown:
                raise SinddmError(f"patch_refine: unknown keys {sorted(unknown)}")
            opt = cls(**opt)
        if not isinstance(opt, cls):
            raise SinddmError(f"patch_refine: a dict or a PatchRefine, got {type(opt).__name__}")
        if not isinstance(opt.iters, int) or opt.iters < 1:
            raise SinddmError(f"patch_refine: iters must be an integer >= 1, got {opt.iters!r}")
        if opt.patch not in PATCHES:
            raise SinddmError(f"patch_refine: patch must be one of {PATCHES}, got {opt.patch!r}")
        check_alpha(opt.alpha)
        check_blend(opt.blend, "patch_refine")
        if opt.scales is not None:
            sc = tuple(opt.scales)
            if len(sc) != 2 or not all(isinstance(v, int) for v in sc) or not 0 <= sc[0] <= sc[1]:
                raise SinddmError(f"patch_refine: scales = (a, b) needs integers 0 <= a <= b, got {opt.scales!r}")
            opt.scales = sc
        return opt

    def covers(self, s: int) -> bool:
        return self.scales is None or self.scales[0] <= int(s) <= self.scales[1]


def check_alpha(alpha) -> Optional[float]:
    if alpha is None:
        return None
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        raise SinddmError(f"patch_refine: alpha must be a number > 0 or None, got {alpha!r}") from None
    if not math.isfinite(a) or a <= 0.0:
        raise SinddmError(f"patch_refine: alpha must be finite and > 0, got {alpha!r}")
    return a


def patch_vote(idx_or_yx: torch.Tensor, ref: torch.Tensor, size: Sequence[int], patch: int, wrap_out=(False, False),
               wrap_ref=(False, False), base: torch.Tensor = None, weight: Optional[torch.Tensor] = None,
               blend: float = 1.0) -> torch.Tensor:
    """The vote of a field.  `idx_or_yx`: (B, h, w) int32 linear positions or (B, 2, h, w) coordinates, as `patch_nnf`
    returns them (a negative entry names no patch); `ref` (B or 1, 3, Hr, Wr) the image the field points into; `size` =
    (H, W) of the result, whose axes wrap as `wrap_out` says (the field's query side); `base` (B, 3, H, W) the image the
    vote is blended into: out = base + g (mean - base) with g = blend * weight, `weight` (B or 1, H, W) or (H, W) or None
    (g = blend); a pixel no patch covers keeps `base`.  Returns a new (B, 3, H, W) tensor."""
    blend = check_blend(blend)
    if patch not in PATCHES:
        raise SinddmError(f"patch_vote: patch must be one of {PATCHES}, got {patch}")
    for name, t in (("field", idx_or_yx), ("ref", ref), ("base", base)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SinddmError(f"patch_vote: {name} must be on a ROCm device (no CPU fallback)")
    H, W = int(size[0]), int(size[1])
    if ref.dim() != 4 or ref.shape[1] != 3 or ref.dtype != torch.float32:
        raise SinddmError(f"patch_vote: ref must be a (B, 3, H, W) float32 tensor, got {tuple(ref.shape)} {ref.dtype}")
    Hr, Wr = int(ref.shape[2]), int(ref.shape[3])
    if min(H, W, Hr, Wr) < patch:
        raise SinddmError(f"patch_vote: an axis of {(H, W)} / {(Hr, Wr)} is shorter than the patch ({patch})")
    h, w = grid_size((H, W), patch, wrap_out)
    hr, wr = grid_size((Hr, Wr), patch, wrap_ref)
    if idx_or_yx.dtype != torch.int32:
        raise SinddmError(f"patch_vote: the field must be int32, got {idx_or_yx.dtype}")
    if idx_or_yx.dim() == 4 and idx_or_yx.shape[1] == 2:
        idx = (idx_or_yx[:, 0] * wr + idx_or_yx[:, 1]).to(torch.int32)        # (-1, wr - 1) -> -1 again
    else:
        idx = idx_or_yx
    if idx.dim() != 3 or tuple(idx.shape[1:]) != (h, w):
        raise SinddmError(f"patch_vote: the field must be (B, {h}, {w}) or (B, 2, {h}, {w}), got {tuple(idx_or_yx.shape)}")
    B = int(idx.shape[0])
    if tuple(base.shape) != (B, 3, H, W) or base.dtype != torch.float32:
        raise SinddmError(f"patch_vote: base must be a ({B}, 3, {H}, {W}) float32 tensor, got {tuple(base.shape)} {base.dtype}")
    if ref.shape[0] not in (1, B) or ref.device != idx.device or base.device != idx.device:
        raise SinddmError(f"patch_vote: a reference batch of {ref.shape[0]} on {ref.device} does not go with the field's {B}")
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or weight.device != idx.device:
            raise SinddmError("patch_vote: weight must be a float32 tensor on the field's device")
        if weight.dim() == 2:
            weight = weight[None]
        if weight.dim() != 3 or tuple(weight.shape[1:]) != (H, W) or weight.shape[0] not in (1, B):
            raise SinddmError(f"patch_vote: weight must be (B or 1, {H}, {W}), got {tuple(weight.shape)}")
        weight = weight.contiguous()
    idx, ref, base = idx.contiguous(), ref.contiguous(), base.contiguous()
    lib = _lib.load()
    with torch.cuda.device(idx.device):
        out = torch.empty_like(base)
        rc = lib.sinddm_patch_vote(_lib.ptr(idx), _lib.ptr(ref), int(ref.shape[0] == B and B > 1), _lib.ptr(base),
                                   _lib.ptr(weight), int(weight is not None and weight.shape[0] == B and B > 1),
                                   _lib.ptr(out), B, H, W, Hr, Wr, patch, _wrap_bits(wrap_out), _wrap_bits(wrap_ref), blend,
                                   _lib.stream_ptr(idx.device))
    _lib.check(rc, "sinddm_patch_vote")
    return out


def patch_refine(x: torch.Tensor, image: torch.Tensor, patch: int = 7, iters: int = 1, alpha: Optional[float] = None,
                 blend: float = 1.0, tile=(False, False), valid: Optional[torch.Tensor] = None,
                 weight: Optional[torch.Tensor] = None, history: bool = False):
    """`iters` field-and-vote iterations of the batch `x` (B, 3, H, W) against the training `image` (3, Hi, Wi), both on
    the device; the sizes may differ.  Every iteration is `(dist, yx) = patch_nnf(x, image)` then
    `x = patch_vote(yx, image, base=x)`, and adds no arithmetic of its own.  `alpha`: the completeness normalisation --
    `m = patch_nnf(image, x)` gives per sample the distance of every image patch to its nearest sample patch and the search
    ranks by dist * 1 / (alpha 3 P^2 + m); `blend`, `weight`: as `patch_vote` takes them; `tile` = (y, x): the axes on which
    the samples wrap around (the image never does); `valid`: an (Hi, Wi) pixel map of the image, 1 = usable -- patches that
    touch the rest are never copied from.  Returns (x, energy): energy (iters, B) float64, the sum of `dist` over the field
    each iteration STARTED from (the patch energy of its input); with `history` also the list of the iterates."""
    blend = check_blend(blend, "patch_refine")
    alpha = check_alpha(alpha)
    if not isinstance(iters, int) or iters < 1:
        raise SinddmError(f"patch_refine: iters must be an integer >= 1, got {iters!r}")
    if image.dim() == 3:
        image = image[None]
    tile = (bool(tile[0]), bool(tile[1]))
    plain = (False, False)
    K = 3 * patch * patch
    energy, iterates = [], []
    for _ in range(iters):
        scale = None
        if alpha is not None:
            m, _yx = patch_nnf(image, x, patch, wrap_query=plain, wrap_ref=tile)
            scale = 1.0 / (alpha * K + m)
        dist, yx = patch_nnf(x, image, patch, wrap_query=tile, wrap_ref=plain, ref_valid=valid, ref_scale=scale)
        energy.append(dist.to(torch.float64).sum(dim=(1, 2)))
        x = patch_vote(yx, image, x.shape[2:], patch, wrap_out=tile, wrap_ref=plain, base=x, weight=weight, blend=blend)
        if history:
            iterates.append(x)
    energy = torch.stack(energy)
    return (x, energy, iterates) if history else (x, energy)
