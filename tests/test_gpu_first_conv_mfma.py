"""GPU: the first conv of the network (3 -> C_out, 3x3, + bias + GELU) on the fp32 matrix cores (conv3x3_c3_mfma_kernel,
csrc/conv_c3m.h) ONE LAUNCH AT A TIME through sinddm_debug_first_conv, against torch's conv2d + erf GELU in float64 on the
CPU; variant 1 is the VALU kernel it replaces in inference (conv3x3_c3_gelu_kernel), variant 2 the new one.

Shapes (B, H, W, Wt, C_out), the smallest that reach each hazard: (1, 3, 4) one partial wave, every pixel on a border;
(2, 5, 64) exactly one wave per row; (2, 7, 68) a second, partial wave per row; (1, 9, 132) with Wt = 130 padded rows, whose
pad columns must come back exactly 0.0; (1, 6, 260) at C_out = 160: ten m-tiles and a fifth, 4-pixel segment per
row; (3, 17, 96) several samples (the maxima are per sample, a persistent wave crosses samples).
Inputs: uniform noise in [-1, 1] (sample 1 of a batch 64 times louder, so that a maximum published to the wrong sample
shows); one case with a single value of 1000 at each of the four corners of every plane over noise of 1e-3: a wrong halo
row or column is an error of order one.  Weights: He-normal, and the closed-form fill of the network's l1.net.0.

Gate (tests/test_gpu_conv_wr.py's): per sample, rel-L2 and max-abs error against float64 of variant 2 <= 1.5 x the larger
of variant 1's and of conv2d + GELU in float32 on the CPU.  Bit for bit: the published maximum is max |out| of the kernel's
own output, a second call repeats the first, grids sized for 1, 8 and 256 compute units agree.
reference SinDDM/models.py:63-64 (l1.net.0 and its GELU)"""
import math

import pytest
import torch
import torch.nn.functional as F

from sinddm_amd.synth import closed_form_state_dict, hash_randn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR = 1.5
BADSHAPE = -2
# (B, H, W, Wt, C_out)
SHAPES = [(1, 3, 4, 0, 80), (2, 5, 64, 0, 80), (2, 7, 68, 0, 80), (1, 9, 132, 130, 80), (1, 6, 260, 0, 160), (3, 17, 96, 0, 80)]
_IDS = [f"{s[0]}x{s[1]}x{s[2]}" + (f"_Wt{s[3]}" if s[3] else "") + f"_co{s[4]}" for s in SHAPES]


def _lib():
    from sinddm_amd import _lib
    return _lib, _lib.load()


def _weights(kind, co, seed):
    if kind == "closed":
        sd = closed_form_state_dict(2 * co)
        return sd["l1.net.0.weight"].clone(), sd["l1.net.0.bias"].clone()
    return hash_randn((co, 3, 3, 3), seed) * math.sqrt(2.0 / 27.0), hash_randn((co,), seed + 1) * 0.05


def _noise(B, H, W, Wt, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 3, H, W), generator=gen) * 2.0 - 1.0
    if B > 1:
        x[1] *= 64.0
    if Wt:
        x[..., Wt:] = 0.0
    return x


def _reference(dt, x, w, bias, Wt):
    v = F.gelu(F.conv2d(x.to(dt), w.to(dt), bias.to(dt), padding=1))
    if Wt:
        v = v.clone()
        v[..., Wt:] = 0.0
    return v


def _run(variant, ncu, x_d, w_d, b_d, Wt=0, expect=0):
    """One launch; returns (out, amax [B]) on the CPU.  `out` starts as NaN, the maxima as zeros."""
    L, lib = _lib()
    B, _, H, W = x_d.shape
    co = w_d.shape[0]
    out = torch.full((B, co, H, W), float("nan"), device=DEV)
    amax = torch.zeros(B, 8, device=DEV)
    rc = lib.sinddm_debug_first_conv(variant, ncu, B, H, W, Wt, co, L.ptr(x_d), L.ptr(w_d), L.ptr(b_d), L.ptr(out), L.ptr(amax),
                                     L.stream_ptr(DEV))
    assert rc == expect, (rc, expect)
    torch.cuda.synchronize(DEV)
    return out.cpu(), amax[:, 0].cpu()


def _errors(got, ref64):
    d = got.double() - ref64
    return [(float(d[b].norm() / ref64[b].norm().clamp_min(1e-300)), float(d[b].abs().max())) for b in range(got.shape[0])]


def _gate(label, got2, got1, ref32, ref64):
    e2, e1, e32 = _errors(got2, ref64), _errors(got1, ref64), _errors(ref32, ref64)
    assert torch.isfinite(got2).all(), label
    for b in range(got2.shape[0]):
        for k, what in enumerate(("rel-L2", "max-abs")):
            yard = max(e1[b][k], e32[b][k])
            print(f"[first_conv] {label} sample {b} {what}: mfma {e2[b][k]:.3e}  valu {e1[b][k]:.3e}  fp32 conv2d {e32[b][k]:.3e}  "
                  f"ratio {e2[b][k] / yard:.3f}")
    for b in range(got2.shape[0]):
        for k, what in enumerate(("rel-L2", "max-abs")):
            assert e2[b][k] <= FACTOR * max(e1[b][k], e32[b][k]), (label, b, what, e2[b], e1[b], e32[b])


@pytest.mark.parametrize("kind", ["he", "closed"])
@pytest.mark.parametrize("B,H,W,Wt,co", SHAPES, ids=_IDS)
def test_against_float64(B, H, W, Wt, co, kind):
    x = _noise(B, H, W, Wt, 4000 + 7 * H + W)
    w, bias = _weights(kind, co, 4100 + H)
    ref64, ref32 = _reference(torch.float64, x, w, bias, Wt), _reference(torch.float32, x, w, bias, Wt)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), bias.to(DEV)
    got2, amax2 = _run(2, 0, x_d, w_d, b_d, Wt)
    got1, amax1 = _run(1, 0, x_d, w_d, b_d, Wt)
    _gate(f"{B}x{H}x{W} co {co} {kind}", got2, got1, ref32, ref64)
    if Wt:
        assert (got2[..., Wt:] == 0).all() and (got1[..., Wt:] == 0).all()
    # the published maximum is that of the kernel's own output, per sample; a second call repeats the first
    assert torch.equal(amax2, got2.abs().amax(dim=(1, 2, 3)))
    assert torch.equal(amax1, got1.abs().amax(dim=(1, 2, 3)))
    again, amax_again = _run(2, 0, x_d, w_d, b_d, Wt)
    assert torch.equal(again, got2) and torch.equal(amax_again, amax2)


def test_large_values_at_the_four_corners():
    B, H, W, co = 2, 7, 68, 80
    x = _noise(B, H, W, 0, 4200) * 1e-3
    for yy in (0, H - 1):
        for xx in (0, W - 1):
            x[:, :, yy, xx] = 1000.0
    w, bias = _weights("he", co, 4210)
    ref64, ref32 = _reference(torch.float64, x, w, bias, 0), _reference(torch.float32, x, w, bias, 0)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), bias.to(DEV)
    got2, _ = _run(2, 0, x_d, w_d, b_d)
    got1, _ = _run(1, 0, x_d, w_d, b_d)
    _gate("corners", got2, got1, ref32, ref64)
    # away from the corners' 2x2 neighbourhoods nothing may see them
    far = torch.ones(H, W, dtype=torch.bool)
    for ys in (slice(0, 2), slice(H - 2, H)):
        for xs in (slice(0, 2), slice(W - 2, W)):
            far[ys, xs] = False
    assert float((got2.double() - ref64)[..., far].abs().max()) < 1e-5


def test_result_does_not_depend_on_the_grid():
    B, H, W, co = 3, 17, 96, 80
    x = _noise(B, H, W, 0, 4300)
    w, bias = _weights("he", co, 4310)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), bias.to(DEV)
    got = {ncu: _run(2, ncu, x_d, w_d, b_d) for ncu in (1, 8, 256, 0)}
    for ncu in (8, 256, 0):
        assert torch.equal(got[ncu][0], got[1][0]) and torch.equal(got[ncu][1], got[1][1]), ncu
    # the library's choice: a launch of 102 segments is below the floor of a 256-CU device, and rows of 96 fill 75 % of their
    # two segments; 3 x 17 x 128 on a 1-CU device is above the floor with whole segments
    assert torch.equal(_run(0, 256, x_d, w_d, b_d)[0], _run(1, 256, x_d, w_d, b_d)[0])
    assert torch.equal(_run(0, 1, x_d, w_d, b_d)[0], _run(1, 1, x_d, w_d, b_d)[0])
    x2 = _noise(B, H, 128, 0, 4320).to(DEV)
    assert torch.equal(_run(0, 1, x2, w_d, b_d)[0], _run(2, 1, x2, w_d, b_d)[0])


@pytest.mark.parametrize("B,H,W,co", [(1, 6, 16, 10), (1, 6, 18, 80), (1, 6, 17, 80)], ids=["co10", "W18", "W17"])
def test_shapes_the_matrix_core_kernel_does_not_take(B, H, W, co):
    x = _noise(B, H, W, 0, 4400)
    w, bias = _weights("he", co, 4410)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), bias.to(DEV)
    out, amax = _run(2, 0, x_d, w_d, b_d, expect=BADSHAPE)
    assert torch.isnan(out).all() and (amax == 0).all()
    # ... and the library's choice for them is the VALU kernel
    got0, got1 = _run(0, 1, x_d, w_d, b_d)[0], _run(1, 1, x_d, w_d, b_d)[0]
    assert torch.equal(got0, got1) and torch.isfinite(got1).all()
