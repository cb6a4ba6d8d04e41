"""The host-side plan of one training step: what `MultiScaleGaussianDiffusion.p_losses` runs.  Plain Python, like
`sampler.RunPlan`: no device work, no library call.  `TrainStep` resolves the loss type, the halo of `train_tile`, the map of
`train_weights` and the two library entries ONCE, before anything is launched; `p_losses` hands it to `_q_sample_impl` and to
the one loss function.  A new training option is one more field here."""
from __future__ import annotations

import torch

from . import _lib
from .autograd import l1_entry

LOSS_TYPES = ('l1', 'l2', 'l1_pred_img')


class TrainStep:
    """One `p_losses` call of the diffusion object `d` on a (B,C,H,W) batch `shape` at scale `s`.  Attributes: `s`, `loss_type`,
    `halo` = (hy, hx) (_lib.TILE_HALO on each axis `d.train_tile` wraps, else 0), `shape` / `ext_shape` (the batch, and the batch
    extended by the halo: what the network sees), `gamma_row` (the row d.gammas[s - 1] for s > 0 -- NOT clamped to 0.55 in
    training -- else None), `weight` / `inv_norm` (the scale's map of `d.train_weights` and 1 / (B C sum w), both None without
    maps), `q_entry` / `loss_entry` (the library entries the step calls; `loss_entry` is None for the two loss types whose loss
    is torch ops).

    Everything is validated here, in this order, so that a defective call is refused before x_noisy is written and before the
    network's forward overwrites the training workspace:
      1. the loss type: NotImplementedError
      2. `train_weights`, SinddmError each: a map for scale s; an (H,W) fp32 tensor; a finite sum > 0
    The sum is taken in float64 on the host once per scale and map OBJECT (one device-to-host copy, cached in
    `d._train_weight_norm`): replace the list entry to change a map."""

    def __init__(self, d, shape, s):
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
        self.q_entry = "sinddm_q_sample_wrap" if hy or hx else "sinddm_q_sample"
        self.loss_entry = l1_entry(self.halo, self.weight is not None) if d.loss_type == 'l1' else None
