"""What a sample copies: the patch nearest-neighbour field (NNF) between samples and the one training image.

For every P x P patch of a query image `patch_nnf` gives the nearest P x P patch of a reference image -- its squared
distance and its coordinates -- through `sinddm_patch_nnf` (csrc/patch_nnf.h: the fp32 matrix pipe with a fused arg-min; the
contract is in include/sinddm_hip.h).  `nnf_stats` turns a field into numbers (plain torch, any device), `patch_report`
runs both directions for a batch of samples:

    fidelity   mean nearest distance per patch element, sample -> image: how plausible the sample's patches are
    coherence  share of positions whose right and lower neighbours were taken from the neighbouring places: 1 for a copy or
               a shift of the image, ~0 for a reshuffle of its patches
    seam       (tiled samples) mean distance of the patches that cross a wrapped border over that of the others
    coverage   mean nearest distance per patch element, image -> sample: how much of the image the sample shows

There is no CPU route: the field of one 186 x 248 sample is 1.9e9 pairs of 147-vectors.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import SinddmError

PATCHES = (3, 5, 7)


def _wrap_bits(wrap: Sequence[bool]) -> int:
    return (1 if wrap[0] else 0) | (2 if wrap[1] else 0)


def grid_size(size: Sequence[int], patch: int, wrap: Sequence[bool]):
    """Patch positions per axis of an (H, W) image: n - P + 1 without wrap, n with it."""
    return tuple(int(n) if w else int(n) - patch + 1 for n, w in zip(size, wrap))


def position_ok(valid: torch.Tensor, patch: int, wrap: Sequence[bool]) -> torch.Tensor:
    """(H, W) pixel map, 1 = usable -> (h, w) fp32 position map: 1 where all P x P pixels of the patch are usable."""
    bad = (valid == 0).to(torch.float32)[None, None]
    if wrap[0]:
        bad = torch.cat([bad, bad[:, :, :patch - 1]], dim=2)
    if wrap[1]:
        bad = torch.cat([bad, bad[:, :, :, :patch - 1]], dim=3)
    return (F.max_pool2d(bad, patch, stride=1)[0, 0] == 0).to(torch.float32).contiguous()


def patch_nnf(query: torch.Tensor, ref: torch.Tensor, patch: int = 7, wrap_query=(False, False), wrap_ref=(False, False),
              ref_valid: Optional[torch.Tensor] = None, ref_scale: Optional[torch.Tensor] = None):
    """Nearest reference patch of every query patch.  `query` (B or 1, 3, Hq, Wq) and `ref` (B or 1, 3, Hr, Wr) are fp32
    device tensors (a batch of 1 is shared by the samples of the other); `wrap_*` = (y, x) says which axes wrap around;
    `ref_valid` is an (Hr, Wr) pixel map, 1 = usable: a reference position is admissible iff all P x P pixels of its patch are.
    `ref_scale` (B or 1, hr, wr) fp32, finite and > 0: rank by max(d, 0) * ref_scale[position] instead of by d
    (`sinddm_patch_nnf_scaled`: GPNN's completeness normalisation); `dist` stays the unscaled distance of the winner.
    Returns (dist (B, hq, wq) fp32: the squared distance to the winner, yx (B, 2, hq, wq) int32: its position)."""
    for name, t in (("query", query), ("ref", ref)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SinddmError(f"patch_nnf: {name} must be on a ROCm device (no CPU fallback)")
        if t.dim() != 4 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise SinddmError(f"patch_nnf: {name} must be a (B, 3, H, W) float32 tensor, got {tuple(t.shape)} {t.dtype}")
    if patch not in PATCHES:
        raise SinddmError(f"patch_nnf: patch must be one of {PATCHES}, got {patch}")
    Bq, Br = query.shape[0], ref.shape[0]
    B = max(Bq, Br)
    if Bq not in (1, B) or Br not in (1, B) or ref.device != query.device:
        raise SinddmError(f"patch_nnf: batches of {Bq} and {Br} on {query.device} / {ref.device} do not go together")
    Hq, Wq, Hr, Wr = query.shape[2], query.shape[3], ref.shape[2], ref.shape[3]
    if min(Hq, Wq, Hr, Wr) < patch:
        raise SinddmError(f"patch_nnf: an axis of {(Hq, Wq)} / {(Hr, Wr)} is shorter than the patch ({patch})")
    hq, wq = grid_size((Hq, Wq), patch, wrap_query)
    hr, wr = grid_size((Hr, Wr), patch, wrap_ref)
    query, ref = query.contiguous(), ref.contiguous()
    ok = None
    if ref_valid is not None:
        if tuple(ref_valid.shape) != (Hr, Wr):
            raise SinddmError(f"patch_nnf: ref_valid must be ({Hr}, {Wr}), got {tuple(ref_valid.shape)}")
        ok = position_ok(ref_valid.to(ref.device), patch, wrap_ref)
        if not bool(ok.any()):
            raise SinddmError("patch_nnf: ref_valid leaves no admissible reference position")
    if ref_scale is not None:
        return _patch_nnf_scaled(query, ref, patch, wrap_query, wrap_ref, ok, ref_scale, B, (hq, wq), (hr, wr))
    lib = _lib.load()
    wq_bits, wr_bits = _wrap_bits(wrap_query), _wrap_bits(wrap_ref)
    nbytes = lib.sinddm_patch_nnf_workspace_bytes(B, Hq, Wq, Hr, Wr, patch, wq_bits, wr_bits)
    if nbytes == 0:
        raise SinddmError(f"patch_nnf: unsupported shape {(B, Hq, Wq)} against {(Hr, Wr)}")
    with torch.cuda.device(query.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
        dist = torch.empty(B, hq, wq, dtype=torch.float32, device=query.device)
        idx = torch.empty(B, hq, wq, dtype=torch.int32, device=query.device)
        rc = lib.sinddm_patch_nnf(_lib.ptr(query), int(Bq == B), _lib.ptr(ref), int(Br == B), _lib.ptr(ok), _lib.ptr(dist),
                                  _lib.ptr(idx), B, Hq, Wq, Hr, Wr, patch, wq_bits, wr_bits, _lib.ptr(ws), nbytes,
                                  _lib.stream_ptr(query.device))
    _lib.check(rc, "sinddm_patch_nnf")
    yx = torch.stack([torch.div(idx, wr, rounding_mode="floor"), idx % wr], dim=1).to(torch.int32)
    return dist, yx


def check_ref_scale(ref_scale, B: int, ref_grid: Sequence[int]) -> torch.Tensor:
    """The precondition of `sinddm_patch_nnf_scaled`, checked here because the entry cannot: a float32 (B or 1, hr, wr) (or
    (hr, wr)) map whose every entry is finite and > 0.  Returns it with the batch dimension."""
    hr, wr = ref_grid
    if not isinstance(ref_scale, torch.Tensor) or ref_scale.dtype != torch.float32:
        raise SinddmError("patch_nnf: ref_scale must be a float32 tensor")
    if ref_scale.dim() == 2:
        ref_scale = ref_scale[None]
    if ref_scale.dim() != 3 or tuple(ref_scale.shape[1:]) != (hr, wr) or ref_scale.shape[0] not in (1, B):
        raise SinddmError(f"patch_nnf: ref_scale must be (B or 1, {hr}, {wr}), got {tuple(ref_scale.shape)}")
    if not bool((torch.isfinite(ref_scale) & (ref_scale > 0)).all()):
        raise SinddmError("patch_nnf: every ref_scale must be finite and > 0")
    return ref_scale


def _patch_nnf_scaled(query, ref, patch, wrap_query, wrap_ref, ok, ref_scale, B, qgrid, rgrid):
    """The scaled route of `patch_nnf` (arguments already checked there)."""
    (hq, wq), (hr, wr) = qgrid, rgrid
    ref_scale = check_ref_scale(ref_scale, B, (hr, wr))
    if ref_scale.device != query.device:
        raise SinddmError("patch_nnf: ref_scale must be on the device of query")
    ref_scale = ref_scale.contiguous()
    Hq, Wq, Hr, Wr = query.shape[2], query.shape[3], ref.shape[2], ref.shape[3]
    lib = _lib.load()
    wq_bits, wr_bits = _wrap_bits(wrap_query), _wrap_bits(wrap_ref)
    nbytes = lib.sinddm_patch_nnf_scaled_workspace_bytes(B, Hq, Wq, Hr, Wr, patch, wq_bits, wr_bits)
    if nbytes == 0:
        raise SinddmError(f"patch_nnf: unsupported shape {(B, Hq, Wq)} against {(Hr, Wr)}")
    with torch.cuda.device(query.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
        dist = torch.empty(B, hq, wq, dtype=torch.float32, device=query.device)
        idx = torch.empty(B, hq, wq, dtype=torch.int32, device=query.device)
        rc = lib.sinddm_patch_nnf_scaled(_lib.ptr(query), int(query.shape[0] == B), _lib.ptr(ref), int(ref.shape[0] == B),
                                         _lib.ptr(ok), _lib.ptr(ref_scale), int(ref_scale.shape[0] == B and B > 1),
                                         _lib.ptr(dist), _lib.ptr(idx), B, Hq, Wq, Hr, Wr, patch, wq_bits, wr_bits,
                                         _lib.ptr(ws), nbytes, _lib.stream_ptr(query.device))
    _lib.check(rc, "sinddm_patch_nnf_scaled")
    yx = torch.stack([torch.div(idx, wr, rounding_mode="floor"), idx % wr], dim=1).to(torch.int32)
    return dist, yx


MAX_RADIUS = 16


def check_radius(radius, what="patch_nnf_local") -> int:
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= MAX_RADIUS:
        raise SinddmError(f"{what}: radius must be an integer in 0 .. {MAX_RADIUS}, got {radius!r}")
    return radius


def patch_nnf_local(query: torch.Tensor, ref: torch.Tensor, prior: torch.Tensor, radius: int, patch: int = 7,
                    wrap_query=(False, False), wrap_ref=(False, False), ref_valid: Optional[torch.Tensor] = None,
                    ref_scale: Optional[torch.Tensor] = None):
    """`patch_nnf` searched in a window: every query patch is compared with the reference positions within `radius` (0 .. 16)
    of its `prior` position only (`sinddm_patch_nnf_local`, csrc/patch_local.h).  `prior`: (B, 2, hq, wq) int32 coordinates
    as `patch_nnf` returns them, or (B, hq, wq) int32 linear positions (its batch may be the only one that is not 1: one
    query searched around several priors); a (-1, .) pair or an entry outside the reference
    grid means "no prior" and gives dist = +inf, yx = (-1, wr - 1) (the linear position -1, as the vote reads it).  The
    other arguments, the ranking with `ref_scale` and the returned (dist, yx) are `patch_nnf`'s; `dist` of a winner is
    bit-equal to what `patch_nnf` reports for the same pair."""
    radius = check_radius(radius)
    for name, t in (("query", query), ("ref", ref)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SinddmError(f"patch_nnf_local: {name} must be on a ROCm device (no CPU fallback)")
        if t.dim() != 4 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise SinddmError(f"patch_nnf_local: {name} must be a (B, 3, H, W) float32 tensor, got {tuple(t.shape)} {t.dtype}")
    if patch not in PATCHES:
        raise SinddmError(f"patch_nnf_local: patch must be one of {PATCHES}, got {patch}")
    if not isinstance(prior, torch.Tensor) or prior.dtype != torch.int32 or prior.device != query.device:
        raise SinddmError("patch_nnf_local: prior must be an int32 tensor on the device of query")
    Bq, Br = query.shape[0], ref.shape[0]
    B = max(Bq, Br, prior.shape[0] if prior.dim() else 1)     # (one query image may be searched around several priors)
    if Bq not in (1, B) or Br not in (1, B) or ref.device != query.device:
        raise SinddmError(f"patch_nnf_local: batches of {Bq} and {Br} on {query.device} / {ref.device} do not go together")
    Hq, Wq, Hr, Wr = query.shape[2], query.shape[3], ref.shape[2], ref.shape[3]
    if min(Hq, Wq, Hr, Wr) < patch:
        raise SinddmError(f"patch_nnf_local: an axis of {(Hq, Wq)} / {(Hr, Wr)} is shorter than the patch ({patch})")
    hq, wq = grid_size((Hq, Wq), patch, wrap_query)
    hr, wr = grid_size((Hr, Wr), patch, wrap_ref)
    if prior.dim() == 4 and prior.shape[1] == 2:
        lin = prior[:, 0] * wr + prior[:, 1]
        off = (prior[:, 0] < 0) | (prior[:, 0] >= hr) | (prior[:, 1] < 0) | (prior[:, 1] >= wr)
        prior = torch.where(off, torch.full_like(lin, -1), lin).to(torch.int32)
    if prior.dim() != 3 or tuple(prior.shape) != (B, hq, wq):
        raise SinddmError(f"patch_nnf_local: prior must be ({B}, {hq}, {wq}) or ({B}, 2, {hq}, {wq}), got {tuple(prior.shape)}")
    query, ref, prior = query.contiguous(), ref.contiguous(), prior.contiguous()
    ok = None
    if ref_valid is not None:
        if tuple(ref_valid.shape) != (Hr, Wr):
            raise SinddmError(f"patch_nnf_local: ref_valid must be ({Hr}, {Wr}), got {tuple(ref_valid.shape)}")
        ok = position_ok(ref_valid.to(ref.device), patch, wrap_ref)
    per_sample_scale = 0
    if ref_scale is not None:
        ref_scale = check_ref_scale(ref_scale, B, (hr, wr))
        if ref_scale.device != query.device:
            raise SinddmError("patch_nnf_local: ref_scale must be on the device of query")
        ref_scale = ref_scale.contiguous()
        per_sample_scale = int(ref_scale.shape[0] == B and B > 1)
    lib = _lib.load()
    with torch.cuda.device(query.device):
        dist = torch.empty(B, hq, wq, dtype=torch.float32, device=query.device)
        idx = torch.empty(B, hq, wq, dtype=torch.int32, device=query.device)
        rc = lib.sinddm_patch_nnf_local(_lib.ptr(query), int(Bq == B), _lib.ptr(ref), int(Br == B), _lib.ptr(ok),
                                        _lib.ptr(ref_scale), per_sample_scale, _lib.ptr(prior), radius, _lib.ptr(dist),
                                        _lib.ptr(idx), B, Hq, Wq, Hr, Wr, patch, _wrap_bits(wrap_query), _wrap_bits(wrap_ref),
                                        _lib.stream_ptr(query.device))
    _lib.check(rc, "sinddm_patch_nnf_local")
    yx = torch.stack([torch.div(idx, wr, rounding_mode="floor"), idx % wr], dim=1).to(torch.int32)
    return dist, yx


def nnf_stats(dist: torch.Tensor, yx: torch.Tensor, patch: int, ref_grid: Sequence[int], wrap_query=(False, False),
              wrap_ref=(False, False)) -> dict:
    """Numbers of a field (`dist` (B, h, w), `yx` (B, 2, h, w)) against a reference grid of `ref_grid` = (hr, wr) positions;
    plain torch on whatever device the field is on.  Per sample, as float64 tensors of B entries:
      fidelity   mean of dist / (3 P^2)
      coherence  share of the positions that have a right and a lower neighbour (on a wrapped query axis the neighbour
                 across the border counts) whose offset yx - (y, x) is the offset of both neighbours; on a wrapped reference
                 axis offsets are compared modulo the reference grid
      seam       only when a query axis wraps: mean dist of the positions whose patch crosses a wrapped border (x > w - P
                 or y > h - P on such an axis) over the mean dist of the others"""
    B, h, w = dist.shape
    d = dist.to(torch.float64)
    out = {"fidelity": d.mean(dim=(1, 2)) / (3 * patch * patch)}
    ys = torch.arange(h, device=yx.device).view(1, h, 1)
    xs = torch.arange(w, device=yx.device).view(1, 1, w)
    off = torch.stack([yx[:, 0].long() - ys, yx[:, 1].long() - xs], dim=1)            # (B, 2, h, w)

    def same(a, b):
        diff = a - b
        eq = torch.ones_like(diff[:, 0], dtype=torch.bool)
        for ax in (0, 1):
            eq &= (diff[:, ax] % int(ref_grid[ax]) == 0) if wrap_ref[ax] else (diff[:, ax] == 0)
        return eq

    right, down = torch.roll(off, -1, dims=3), torch.roll(off, -1, dims=2)
    coh = same(off, right) & same(off, down)
    has = torch.ones(h, w, dtype=torch.bool, device=yx.device)
    if not wrap_query[0]:
        has[h - 1:, :] = False
    if not wrap_query[1]:
        has[:, w - 1:] = False
    n = int(has.sum())
    out["coherence"] = ((coh & has).sum(dim=(1, 2)).to(torch.float64) / n if n else
                        torch.full((B,), float("nan"), dtype=torch.float64, device=dist.device))
    if wrap_query[0] or wrap_query[1]:
        cross = torch.zeros(h, w, dtype=torch.bool, device=dist.device)
        if wrap_query[0]:
            cross |= (ys[0] > h - patch).expand(h, w).to(dist.device)
        if wrap_query[1]:
            cross |= (xs[0] > w - patch).expand(h, w).to(dist.device)
        nc, no = int(cross.sum()), int((~cross).sum())
        on = (d * cross).sum(dim=(1, 2)) / max(nc, 1)
        offm = (d * ~cross).sum(dim=(1, 2)) / max(no, 1)
        out["seam"] = on / offm
    return out


def patch_report(samples: torch.Tensor, image: torch.Tensor, patch: int = 7, tile=(False, False),
                 valid: Optional[torch.Tensor] = None) -> dict:
    """The field in both directions for a batch of `samples` (B, 3, H, W) against the training `image` (3, Hi, Wi), both on
    the device; the sizes may differ (a stretched sample).  `tile` = (y, x): the axes on which the samples wrap around (the
    image never does); `valid`: an (Hi, Wi) pixel map of the image, 1 = usable -- patches that touch the rest are neither
    copied from (sample -> image) nor asked for (image -> sample).  Returns a dict of per-sample lists (`fidelity`,
    `coherence`, `coverage`, and `seam` for tiled samples) and their means (`<name>_mean`)."""
    if image.dim() == 3:
        image = image[None]
    tile = (bool(tile[0]), bool(tile[1]))
    dist, yx = patch_nnf(samples, image, patch, wrap_query=tile, wrap_ref=(False, False), ref_valid=valid)
    ref_grid = grid_size(image.shape[2:], patch, (False, False))
    stats = nnf_stats(dist, yx, patch, ref_grid, wrap_query=tile, wrap_ref=(False, False))
    back, _ = patch_nnf(image, samples, patch, wrap_query=(False, False), wrap_ref=tile)
    back = back.to(torch.float64)
    if valid is not None:
        ok = position_ok(valid.to(back.device), patch, (False, False)).to(torch.float64)
        cover = (back * ok).sum(dim=(1, 2)) / ok.sum()
    else:
        cover = back.mean(dim=(1, 2))
    stats["coverage"] = cover / (3 * patch * patch)
    report = {"patch": int(patch), "samples": int(samples.shape[0]), "tile": [tile[0], tile[1]],
              "sample_size": [int(samples.shape[2]), int(samples.shape[3])],
              "image_size": [int(image.shape[2]), int(image.shape[3])]}
    for name in ("fidelity", "coherence", "seam", "coverage"):
        if name in stats:
            vals = [float(v) for v in stats[name].cpu()]
            report[name] = vals
            report[name + "_mean"] = sum(vals) / len(vals)
    return report
