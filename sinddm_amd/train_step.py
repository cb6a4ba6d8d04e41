"""The host-side plan of one training step: what `MultiScaleGaussianDiffusion.p_losses` runs.  Plain Python, like
`sampler.RunPlan`: no device work, no library call.  `TrainStep` resolves the loss type, the halo of `train_tile`, the map of
`train_weights` and the two library entries ONCE, before anything is launched; `p_losses` hands it to `_q_sample_impl` and to
the one loss function.  A new training option is one more field here."""
from __future__ import annotations

import torch

from . import _lib
from .autograd import l1_entry
from .functions import crop_norm, crop_rects, crop_window, summed_area_table

LOSS_TYPES = ('l1', 'l2', 'l1_pred_img')
CROP_REDRAWS = 16             # how often a cropped step draws again when its windows hold no weight under a mask


class TrainStep:
    """One `p_losses` call of the diffusion object `d` on a (B,C,H,W) batch `shape` at scale `s`.  Attributes: `s`, `loss_type`,
    `halo` = (hy, hx) (_lib.TILE_HALO on each axis `d.train_tile` wraps, else 0), `shape` / `ext_shape` (the batch, and the batch
    extended by the halo: what the network sees), `gamma_row` (the row d.gammas[s - 1] for s > 0 -- NOT clamped to 0.55 in
    training -- else None), `weight` / `inv_norm` (the scale's map of `d.train_weights` and 1 / (B C sum w), both None without
    maps), `q_entry` / `loss_entry` (the library entries the step calls; `loss_entry` is None for the two loss types whose loss
    is torch ops).  Under `d.train_crop` (crop training): `crop` = the scale's window (h, w), or None when the
    window spans the scale -- the step is then today's step, field by field; `windows` / `rects` = the CPU int32 (B,2) origins
    and (B,4) valid rectangles (functions.crop_rects), None without a crop; `ext_shape` is then (B,C,h,w), `inv_norm` is
    1 / (C * functions.crop_norm) whether or not there is a map, and the entries are `sinddm_q_sample_crop` /
    `sinddm_l1_loss_rect_fwd_bwd`.  The origins come from the `windows` argument, else from `draw()` (a callable that returns
    a (B,2) table: `d.crop_fn` or the clamped draw, wrapped by p_losses).  `tables(device)` uploads the two tables.

    Everything is validated here, in this order, so that a defective call is refused before x_noisy is written and before the
    network's forward overwrites the training workspace:
      1. the loss type: NotImplementedError
      2. `train_weights`, SinddmError each: a map for scale s; an (H,W) fp32 tensor; a finite sum > 0
    The sum is taken in float64 on the host once per scale and map OBJECT (one device-to-host copy, cached in
    `d._train_weight_norm`): replace the list entry to change a map.
      3. `train_crop`, SinddmError each, in this order: a `train_crop` that is not two positive integers or a negative
         `train_crop_margin`; `train_crop` together with `train_tile` on any axis (whatever the scale); then, only at a scale
         larger than the crop: a cropped axis whose window is <= 2 margins; origins that are not an integer (B,2) table inside
         0 .. H - h, 0 .. W - w; windows whose valid rectangles hold no weight at all under the map -- a drawn batch is drawn
         again up to CROP_REDRAWS times first, explicit `windows` are refused at once.
    The map's float64 summed-area table is built on the host once per scale and map object (`d._train_crop_sat`)."""

    def __init__(self, d, shape, s, windows=None, draw=None):
        s = self.s = int(s)
        self.loss_type = d.loss_type
        if d.loss_type not in LOSS_TYPES:
            raise NotImplementedError()
        B, Cc, H, W = self.shape = tuple(int(v) for v in shape)
        hy, hx = self.halo = (_lib.TILE_HALO if d.train_tile[0] else 0, _lib.TILE_HALO if d.train_tile[1] else 0)
        self.ext_shape = (B, Cc, H + 2 * hy, W + 2 * hx)
        self.gamma_row = d.gammas[s - 1].reshape(-1).contiguous() if s > 0 else None
        self.weight = self.inv_norm = None
        if d.train_weights is not None:
            if s >= len(d.train_weights):
                raise _lib.SinddmError(f"train_weights holds {len(d.train_weights)} maps: none for scale {s}")
            w = d.train_weights[s]
            if not torch.is_tensor(w) or tuple(w.shape) != (H, W) or w.dtype != torch.float32:
                raise _lib.SinddmError(f"train_weights[{s}] must be a {(H, W)} fp32 tensor, got "
                                       f"{tuple(w.shape) if torch.is_tensor(w) else type(w).__name__}")
            hit = d._train_weight_norm.get(s)
            if hit is None or hit[0] is not w:
                total = float(w.detach().to("cpu", torch.float64).sum())
                if not (total > 0.0 and total < float("inf")):
                    raise _lib.SinddmError(f"train_weights[{s}] sums to {total}: scale {s} has no pixel to train on")
                hit = d._train_weight_norm[s] = (w, total)
            self.weight, self.inv_norm = w, 1.0 / (B * Cc * hit[1])
        self.crop = self.windows = self.rects = None
        if getattr(d, "train_crop", None) is not None:
            self._plan_crop(d, windows, draw)
        if self.crop is not None:
            self.q_entry = "sinddm_q_sample_crop"
        else:
            self.q_entry = "sinddm_q_sample_wrap" if hy or hx else "sinddm_q_sample"
        self.loss_entry = l1_entry(self.halo, self.weight is not None, self.crop is not None) if d.loss_type == 'l1' else None

    def _plan_crop(self, d, windows, draw):
        """Validation 3 of the class docstring, and the crop fields."""
        B, Cc, H, W = self.shape
        crop, m = d.train_crop, d.train_crop_margin
        try:
            crop, m = (int(crop[0]), int(crop[1])), int(m)
            ok = len(d.train_crop) == 2 and crop[0] > 0 and crop[1] > 0 and m >= 0
        except (TypeError, ValueError, IndexError):
            ok = False
        if not ok:
            raise _lib.SinddmError(f"train_crop must be two positive integers and train_crop_margin >= 0, got "
                                   f"{d.train_crop!r} / {d.train_crop_margin!r}")
        if self.halo[0] or self.halo[1]:
            raise _lib.SinddmError("train_crop together with train_tile: wrapped windows are not built")
        h, w = crop_window((H, W), crop)
        if (h, w) == (H, W):
            return                                                           # the scale trains whole: today's step
        for n, k, axis in ((H, h, "y"), (W, w, "x")):
            if k < n and k <= 2 * m:
                raise _lib.SinddmError(f"train_crop: the {k}-pixel window on {axis} at scale {self.s} is not larger than two "
                                       f"margins of {m}")
        sat = None
        if self.weight is not None:
            hit = d._train_crop_sat.get(self.s)
            if hit is None or hit[0] is not self.weight:
                hit = d._train_crop_sat[self.s] = (self.weight, summed_area_table(self.weight))
            sat = hit[1]
        explicit = windows is not None
        if not explicit and draw is None:
            raise _lib.SinddmError(f"train_crop: scale {self.s} is cropped and the step has neither windows nor a draw")
        for _ in range(1 if explicit else 1 + CROP_REDRAWS):
            win = windows if explicit else draw()
            if not torch.is_tensor(win):
                win = torch.as_tensor(win)
            if win.is_floating_point() or win.dtype == torch.bool or tuple(win.shape) != (B, 2):
                raise _lib.SinddmError(f"train_crop: the window origins must be an integer {(B, 2)} table, got "
                                       f"{win.dtype} {tuple(win.shape)}")
            win = win.detach().to("cpu", torch.int64)
            if bool((win < 0).any()) or bool((win[:, 0] > H - h).any()) or bool((win[:, 1] > W - w).any()):
                raise _lib.SinddmError(f"train_crop: window origins {win.tolist()} leave 0..{H - h}, 0..{W - w} at scale {self.s}")
            rects = crop_rects(win, (H, W), crop, m)
            total = crop_norm(win, rects, sat)
            if total > 0.0 and total < float("inf"):
                break
        else:
            raise _lib.SinddmError(f"train_crop: the valid rectangles of scale {self.s} hold no weight under train_weights"
                                   + ("" if explicit else f" in {1 + CROP_REDRAWS} draws"))
        self.crop, self.windows, self.rects = (h, w), win.to(torch.int32).contiguous(), rects.to(torch.int32).contiguous()
        self.ext_shape = (B, Cc, h, w)
        self.inv_norm = 1.0 / (Cc * total)

    def tables(self, device):
        """(windows, rects) as int32 tensors on `device`: one pinned staging buffer, copied without blocking the host."""
        both = torch.stack([self.windows.reshape(-1), self.rects[:, :2].reshape(-1), self.rects[:, 2:].reshape(-1)])
        if torch.device(device).type == "cuda":                              # (3, 2B): one copy, two contiguous views
            both = both.pin_memory().to(device, non_blocking=True)
        B = self.shape[0]
        return both[0].view(B, 2), both[1:].view(2, B, 2).permute(1, 0, 2).reshape(B, 4)
