"""Shared by tests/test_score_host.py and tests/test_gpu_score.py: the denoising score of include/sinddm_hip.h ("denoising-score
maps") restated in float64 on top of oracle/sinddm_oracle.py, and the level sum in numpy.

The restatement takes the draws as an argument: the GPU tests read the device's own draws back (sinddm_normal_fill /
sinddm_normal_fill_samples at the call's stream ids) and replay them here, so the generator is not part of what is compared."""
import numpy as np
import torch

from fullrank_util import net_forward_f64
from oracle import sinddm_oracle as O


def score_f64(sched, sd, y, y_prev, s, levels, draws, weight=None):
    """(map (B,H,W), level (n,B)) in float64.  y / y_prev: (B,3,H,W) fp32 (y_prev None at scale 0); levels: n ints; draws:
    (n,B,3,H,W) fp32, z_i of evaluation i; weight: (H,W) or None.  Evaluation i:
        x_t  = O.p_losses_inputs(x_start = y_prev (y at scale 0), x_orig = y, t_i, z_i)      training's mix, gamma not clamped
        eps  = the oracle's network in float64 on x_t
        m    = w * sum_c |z_i - eps|;     map += m;     level[i] = sum_p m"""
    B, _, H, W = y.shape
    s = int(s)
    sc = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sched.items()}
    w = torch.ones(H, W, dtype=torch.float64) if weight is None else weight.double()
    smap = torch.zeros(B, H, W, dtype=torch.float64)
    level = torch.zeros(len(levels), B, dtype=torch.float64)
    for i, t in enumerate(levels):
        tt = torch.full((B,), int(t), dtype=torch.long)
        z = draws[i].double()
        x_start = y_prev.double() if s > 0 else y.double()
        x_t = O.p_losses_inputs(sc, x_start, tt, s, z, y.double() if s > 0 else None)
        eps = net_forward_f64(sd, x_t, tt, s)
        m = w * (z - eps).abs().sum(dim=1)
        smap += m
        level[i] = m.sum(dim=(1, 2))
    return smap, level


def level_sum_f64(m):
    """The level sum of one evaluation: the float64 sum over the pixels of the fp32 values m (B,H,W) that went into the map."""
    return np.asarray(m, dtype=np.float32).astype(np.float64).reshape(m.shape[0], -1).sum(axis=1)


def dilate(mask, r):
    """A (H,W) bool mask grown by r pixels in the Chebyshev metric (the network's receptive field is a square)."""
    m = torch.as_tensor(mask, dtype=torch.float32)[None, None]
    return torch.nn.functional.max_pool2d(m, 2 * r + 1, stride=1, padding=r)[0, 0] > 0
