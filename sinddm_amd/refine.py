"""Acting on the patch nearest-neighbour field: the patch vote, and the refinement loop built from field and vote.

`metrics.patch_nnf` says which patch of the training image every patch of a sample is nearest to; `patch_vote` replaces
every patch by that one and makes every pixel the mean of the patches that cover it (`sinddm_patch_vote`,
csrc/patch_vote.h; the contract is in include/sinddm_hip.h).  Field then vote is the EM step of GPNN ("Drop the GAN"):
coordinate descent on the patch energy E(x) = sum_i min_j |P_i x - b_j|^2, so with blend = 1 and the plain field the
energy cannot rise.  `patch_refine` iterates it, optionally with GPNN's completeness normalisation (`alpha`): the search
then ranks by D_ij / (alpha 3 P^2 + min_i D_ij) (`sinddm_patch_nnf_scaled`), which pulls the sample towards showing every
patch of the image.  With a `radius` only the first field is searched exhaustively: every later one is searched in a window
around the previous one (`metrics.patch_nnf_local`), and `carry_field` takes a field from one scale of the pyramid to the
next, so a refinement costs what its windows cost.  There is no CPU route.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import SinddmError
from .metrics import PATCHES, _wrap_bits, check_radius, grid_size, patch_nnf, patch_nnf_local


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
    `patch` after the chain of every scale in `scales` = (a, b), inclusive (None: every scale); `alpha`, `blend` and
    `radius` (None: every search exhaustive) as `patch_refine` takes them."""
    iters: int = 1
    patch: int = 7
    alpha: Optional[float] = None
    blend: float = 1.0
    scales: Optional[Tuple[int, int]] = None
    radius: Optional[int] = None

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
        if opt.radius is not None:
            check_radius(opt.radius, "patch_refine")
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


def carry_field(yx: torch.Tensor, patch: int, q_from: Sequence[int], q_to: Sequence[int], r_from: Sequence[int],
                r_to: Sequence[int], wrap_query=(False, False)) -> torch.Tensor:
    """Carry a field from one (sample size, image size) pair to another by patch centres: the prior of the next scale.
    `yx` (B, 2, h, w) int32 as `patch_nnf` returns it for samples of size `q_from` = (H, W) against an unwrapped image of
    size `r_from`; the result is (B, 2, h', w') int32 for samples of size `q_to` against an image of size `r_to`.  Per axis,
    with c = (P - 1) / 2 and pixel centres at integer + 1/2: the new query position y' has its centre at
    u = (y' + c + 1/2) n_from / n_to - 1/2 of the old sample; the old field is read at y = round(u - c), clamped into the old
    grid (taken modulo it on a wrapped query axis); the reference centre it names, r + c, and the query's own offset u - (y + c)
    are mapped by the image-size ratio, r' = round((r + c + 1/2 + u - y - c) m_to / m_from - 1/2 - c), clamped into the new
    reference grid.  float64 on the field's device, deterministic; an entry that names no patch stays (-1, w_ref' - 1), the
    linear position -1; equal sizes give the field back."""
    if patch not in PATCHES:
        raise SinddmError(f"carry_field: patch must be one of {PATCHES}, got {patch}")
    if not isinstance(yx, torch.Tensor) or yx.dtype != torch.int32 or yx.dim() != 4 or yx.shape[1] != 2:
        raise SinddmError("carry_field: the field must be a (B, 2, h, w) int32 tensor")
    sizes = [tuple(int(v) for v in sz) for sz in (q_from, q_to, r_from, r_to)]
    if any(len(sz) != 2 or min(sz) < patch for sz in sizes):
        raise SinddmError(f"carry_field: every size must be (H, W) with both axes >= the patch ({patch}), got {sizes}")
    q_from, q_to, r_from, r_to = sizes
    wrap_query = (bool(wrap_query[0]), bool(wrap_query[1]))
    g_from, g_to = grid_size(q_from, patch, wrap_query), grid_size(q_to, patch, wrap_query)
    gr_from, gr_to = grid_size(r_from, patch, (False, False)), grid_size(r_to, patch, (False, False))
    if tuple(yx.shape[2:]) != g_from:
        raise SinddmError(f"carry_field: a field of {tuple(yx.shape[2:])} does not belong to samples of {q_from} (grid {g_from})")
    c = (patch - 1) / 2.0
    dev = yx.device
    look, off = [], []
    for a in range(2):
        u = (torch.arange(g_to[a], dtype=torch.float64, device=dev) + (c + 0.5)) * (q_from[a] / q_to[a]) - 0.5
        y = torch.floor(u - c + 0.5).to(torch.int64)
        if not wrap_query[a]:
            y = y.clamp(0, g_from[a] - 1)
        off.append(u - y.to(torch.float64) - c)          # (the offset is that of the position before it is wrapped)
        look.append(y % g_from[a])
    old = yx[:, :, look[0][:, None], look[1][None, :]].to(torch.int64)          # (B, 2, h', w')
    none = (old[:, 0] < 0) | (old[:, 0] >= gr_from[0]) | (old[:, 1] < 0) | (old[:, 1] >= gr_from[1])
    out = []
    for a in range(2):
        o = off[a][:, None] if a == 0 else off[a][None, :]
        r = (old[:, a].to(torch.float64) + (c + 0.5) + o) * (r_to[a] / r_from[a]) - 0.5 - c
        out.append(torch.floor(r + 0.5).to(torch.int64).clamp(0, gr_to[a] - 1))
    out[0] = torch.where(none, torch.full_like(out[0], -1), out[0])
    out[1] = torch.where(none, torch.full_like(out[1], gr_to[1] - 1), out[1])
    return torch.stack(out, dim=1).to(torch.int32)


def patch_refine(x: torch.Tensor, image: torch.Tensor, patch: int = 7, iters: int = 1, alpha: Optional[float] = None,
                 blend: float = 1.0, tile=(False, False), valid: Optional[torch.Tensor] = None,
                 weight: Optional[torch.Tensor] = None, history: bool = False, radius: Optional[int] = None,
                 prior: Optional[torch.Tensor] = None, field: bool = False):
    """`iters` field-and-vote iterations of the batch `x` (B, 3, H, W) against the training `image` (3, Hi, Wi), both on
    the device; the sizes may differ.  Every iteration is `(dist, yx) = patch_nnf(x, image)` then
    `x = patch_vote(yx, image, base=x)`, and adds no arithmetic of its own.  `alpha`: the completeness normalisation --
    `m = patch_nnf(image, x)` gives per sample the distance of every image patch to its nearest sample patch and the search
    ranks by dist * 1 / (alpha 3 P^2 + m); `blend`, `weight`: as `patch_vote` takes them; `tile` = (y, x): the axes on which
    the samples wrap around (the image never does); `valid`: an (Hi, Wi) pixel map of the image, 1 = usable -- patches that
    touch the rest are never copied from.
    `radius` (0 .. 16; None: every search exhaustive, the call as it always was): the first iteration searches around
    `prior` (a field as `patch_nnf_local` takes it) if one is given and exhaustively otherwise; every later iteration
    searches the window of `radius` around the previous iteration's field (`patch_nnf_local`, same `valid` and scale).  The
    window contains the previous assignment, so with blend = 1 and no `alpha` the energy still cannot rise.  A query left
    without a patch is skipped by the vote and adds nothing to the energy.  With `alpha` the reverse field `m` stays
    exhaustive (a windowed completeness term is not built).
    Returns (x, energy): energy (iters, B) float64, the sum of `dist` over the field each iteration STARTED from (the patch
    energy of its input); with `history` also the list of the iterates; with `field` also the last iteration's `yx`."""
    blend = check_blend(blend, "patch_refine")
    alpha = check_alpha(alpha)
    if not isinstance(iters, int) or iters < 1:
        raise SinddmError(f"patch_refine: iters must be an integer >= 1, got {iters!r}")
    if radius is not None:
        radius = check_radius(radius, "patch_refine")
    elif prior is not None:
        raise SinddmError("patch_refine: a prior needs a radius")
    if image.dim() == 3:
        image = image[None]
    tile = (bool(tile[0]), bool(tile[1]))
    plain = (False, False)
    K = 3 * patch * patch
    energy, iterates, yx = [], [], None
    for k in range(iters):
        scale = None
        if alpha is not None:
            m, _yx = patch_nnf(image, x, patch, wrap_query=plain, wrap_ref=tile)
            scale = 1.0 / (alpha * K + m)
        around = None if radius is None else (prior if k == 0 else yx)
        if around is None:
            dist, yx = patch_nnf(x, image, patch, wrap_query=tile, wrap_ref=plain, ref_valid=valid, ref_scale=scale)
        else:
            dist, yx = patch_nnf_local(x, image, around, radius, patch, wrap_query=tile, wrap_ref=plain, ref_valid=valid,
                                       ref_scale=scale)
            dist = torch.where(yx[:, 0] < 0, torch.zeros_like(dist), dist)
        energy.append(dist.to(torch.float64).sum(dim=(1, 2)))
        x = patch_vote(yx, image, x.shape[2:], patch, wrap_out=tile, wrap_ref=plain, base=x, weight=weight, blend=blend)
        if history:
            iterates.append(x)
    energy = torch.stack(energy)
    return (x, energy) + ((iterates,) if history else ()) + ((yx,) if field else ())
