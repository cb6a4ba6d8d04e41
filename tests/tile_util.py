"""Shared by tests/test_tile_host.py and tests/test_gpu_tile.py: the oracle with circular padding.

The reference gets a tileable network by setting padding_mode='circular' on its nn.Conv2d's.  The oracle
(oracle/sinddm_oracle.py) calls F.conv2d with zero padding; `circular_oracle(wrap)` patches that one function, for the
duration of a `with` block, so that every padded convolution pads circularly on the wrapped axes (and with zeros on the
others).  The oracle itself is not edited."""
import contextlib
from unittest import mock

import torch
import torch.nn.functional as F

from oracle import sinddm_oracle as O

HALO = 16          # SINDDM_TILE_HALO


@contextlib.contextmanager
def circular_oracle(wrap=(True, True)):
    real = F.conv2d

    def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        p = int(padding)
        if p:
            py, px = (p if wrap[0] else 0), (p if wrap[1] else 0)
            if py or px:
                x = F.pad(x, (px, px, py, py), mode="circular")
            if p - py or p - px:
                x = F.pad(x, (p - px, p - px, p - py, p - py))
        return real(x, w, b, stride, 0, dilation, groups)

    with mock.patch.object(O.F, "conv2d", conv2d):
        yield


def wrap_pad(t, hy, hx):
    """(..., H, W) -> (..., H + 2 hy, W + 2 hx) by modulo indexing (a halo may be wider than the image)."""
    H, W = t.shape[-2], t.shape[-1]
    iy = (torch.arange(-hy, H + hy, device=t.device) % H)
    ix = (torch.arange(-hx, W + hx, device=t.device) % W)
    return t[..., iy[:, None], ix[None, :]].contiguous()


def centre(t, hy, hx):
    H, W = t.shape[-2] - 2 * hy, t.shape[-1] - 2 * hx
    return t[..., hy:hy + H, hx:hx + W].contiguous()
