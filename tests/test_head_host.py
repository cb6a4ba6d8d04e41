"""CPU: the algebra of the collapsed inference head (csrc/head.h) and its place in the packed image.

Block 4 ends in  out = conv2(g) + res(x_in) + biases  and final_conv is a linear 80 -> 3 map of it, so
    eps = conv3x3(g; W_c) + conv1x1(x_in; W_r) + b_c
with W_c = W_f . W_2, W_r = W_f . W_res, b_c = W_f . (b_2 + b_res) + b_f.  Everything here is float64: it checks the
composition and the bias folding, borders included (zero padding commutes with the composition), not rounding.
reference SinDDM/models.py:69-80 (the block), :130-132,151 (final_conv)
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import sinddm_oracle as O
from sinddm_amd.synth import closed_form_state_dict, hash_randn

# sinddm_packed_count before the head's regions existed (the image then ended with its 64-float zero page)
PACKED_BEFORE = {32: 134208, 160: 8628160}


def compose_head(sd):
    """(W_c (3, half, 3, 3), W_r (3, dim, 1, 1), b_c (3,)) in float64 from a state dict."""
    wf = sd["final_conv.0.weight"].double()[:, :, 0, 0]                      # (3, half)
    w2 = sd["l4.net.2.weight"].double()                                      # (half, half, 3, 3)
    wres = sd["l4.res_conv.weight"].double()[:, :, 0, 0]                     # (half, dim)
    wc = torch.einsum("om,mcyx->ocyx", wf, w2)
    wr = (wf @ wres)[:, :, None, None]
    bc = wf @ (sd["l4.net.2.bias"].double() + sd["l4.res_conv.bias"].double()) + sd["final_conv.0.bias"].double()
    return wc, wr, bc


def block4_inputs_f64(sd, x, t, scale):
    """(g, x_in, eps) of the oracle's network in float64: block 4's GELU(conv1) and input, and the network's output."""
    cond = O.cond_vector(sd, t, scale).double()
    sd64 = {k: v.double() for k, v in sd.items()}
    h = x.double()
    for name in ("l1", "l2", "l3"):
        h = O.conv_block(sd64, name, h, cond)
    out, mid = O.conv_block(sd64, "l4", h, cond, return_intermediates=True)
    eps = F.conv2d(out, sd64["final_conv.0.weight"], sd64["final_conv.0.bias"])
    return mid["g"], h, eps


@pytest.mark.parametrize("dim", [32, 160])
def test_collapsed_formula_equals_the_network_in_float64(dim):
    sd = closed_form_state_dict(dim)
    B, H, W = 2, 9, 12
    x = hash_randn((B, 3, H, W), 77) * 0.9
    t = torch.tensor([53, 700], dtype=torch.long)
    g, x_in, eps = block4_inputs_f64(sd, x, t, 2)
    assert g.dtype == x_in.dtype == eps.dtype == torch.float64
    wc, wr, bc = compose_head(sd)
    got = F.conv2d(g, wc, None, padding=1) + F.conv2d(x_in, wr, bc)
    scale = float(eps.abs().max())
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    err = (got - eps).abs()
    print(f"dim {dim}: collapsed vs network, float64: max-abs / max|eps| ring {float(err[..., ring].max()) / scale:.2e} "
          f"interior {float(err[..., ~ring].max()) / scale:.2e}")
    assert float(err[..., ring].max()) <= 1e-12 * scale
    assert float(err[..., ~ring].max()) <= 1e-12 * scale
    # the bias folding is part of it: without b_c the two are O(bias) apart
    assert float((got - bc.view(1, 3, 1, 1) - eps).abs().max()) > 1e-6 * scale


@pytest.mark.parametrize("dim", [32, 160])
def test_packed_image_grows_by_exactly_the_three_regions(dim):
    from sinddm_amd import _lib
    lib = _lib.load()
    half = dim // 2
    off = (C.c_int64 * 3)()
    assert lib.sinddm_debug_head_offsets(dim, off) == 0
    before = PACKED_BEFORE[dim]
    assert off[0] >= before                                                  # behind every older region (none moved)
    assert list(off) == [before, before + half * 27, before + half * 27 + dim * 3]
    assert lib.sinddm_packed_count(dim) == before + half * 27 + dim * 3 + 3
    assert lib.sinddm_debug_head_offsets(3, off) == -1 and lib.sinddm_debug_head_offsets(dim, None) == -1
    # the option bit of `dim` changes no layout
    off2 = (C.c_int64 * 3)()
    assert lib.sinddm_debug_head_offsets(dim | _lib.DIM_FP32_CONVS, off2) == 0 and list(off2) == list(off)


def test_head_path_follows_the_row_alignment():
    from sinddm_amd import _lib
    lib = _lib.load()
    # dim 160 / 32 pad their rows: every width; dim 20 keeps plain rows: W % 4 == 0 only
    for dim, W, want in ((160, 512, 1), (160, 17, 1), (32, 45, 1), (20, 12, 1), (20, 13, 0), (20, 177, 0)):
        assert lib.sinddm_debug_head_path(dim, 2, 9, W) == want, (dim, W)
        assert lib.sinddm_debug_head_path(dim | _lib.DIM_FP32_CONVS, 2, 9, W) == want, (dim, W)
    assert lib.sinddm_debug_head_path(160, 0, 9, 12) == -1
    # argument validation happens before any device work
    assert lib.sinddm_debug_head(None, None, None, None, 160, 1, 8, 8, 8, None) == -1
