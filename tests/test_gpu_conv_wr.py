"""GPU: conv_wh's 160-channel kernel (conv_wr_kernel: items of 8x32 pixels x 160 output channels, a multiplying wave keeps
the two output rows) ONE LAUNCH AT A TIME through sinddm_debug_conv_wh, against torch's conv2d in float64 on the CPU plus
the epilogue in float64.

Shapes, the smallest that reach each hazard: (2, 9, 36) partial tile rows and columns, (1, 5, 4) a plane smaller than one
tile, (3, 24, 64) whole tiles and several tiles per XCD, (2, 16, 68) a 4-pixel last tile column; C_in = 32 the two-chunk
minimum, 48 an odd chunk count (the V-buffer parity flips between the items of a workgroup), 160 the production depth;
C_out = 160 one item per tile, 320 two.  Grids of 8 and 256 compute units at (3, 24, 64) x 320 channels: with 8, one
workgroup per XCD runs six items back to back (item-stream boundary, exchange-buffer placement at both parities).
Inputs: hash_randn, He-normal weights; where the batch has two samples or more, sample 1 is 2^12 louder than the rest;
one case has per-channel gains 2^U(-6, 6) on the weights' input and output channels.

Gate (the project's own, test_gpu_h2.py): per sample, the kernel's rel-L2 and max-abs error against float64 <= 1.5 x the
larger of the 80-channel kernel's error on the same inputs and the error of conv2d in float32 on the CPU.  Per sample,
because a whole-batch norm would see the loud sample only.  Bit for bit: the library's choice = the 160-channel
kernel where C_out % 160 == 0 and the 80-channel kernel elsewhere, 8 and 256 compute units agree, a second call repeats
the first.
reference SinDDM/models.py:63,65 (the 3x3 convolutions), :79-80 (GELU, the residual)"""
import math

import pytest
import torch
import torch.nn.functional as F

from sinddm_amd.synth import hash_randn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR = 1.5
SHAPES = [(2, 9, 36), (1, 5, 4), (3, 24, 64), (2, 16, 68)]


def _lib():
    from sinddm_amd import _lib
    return _lib, _lib.load()


def _inputs(B, H, W, ci, co, seed, gains=False, Wt=0):
    x = hash_randn((B, ci, H, W), seed)
    if B > 1:
        x[1] *= 4096.0
    w = hash_randn((co, ci, 3, 3), seed + 1) * math.sqrt(2.0 / (9 * ci))
    if gains:
        gen = torch.Generator().manual_seed(seed)
        w *= torch.exp2((torch.rand(co, generator=gen) * 2 - 1) * 6).view(-1, 1, 1, 1)
        gi = torch.exp2((torch.rand(ci, generator=gen) * 2 - 1) * 6)
        w /= gi.view(1, -1, 1, 1)
        x *= gi.view(1, -1, 1, 1)
    if Wt:
        x[..., Wt:] = 0.0
    return x, w, hash_randn((co,), seed + 2) * 0.1


def _gelu_grad(a):
    return 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


def _reference(dt, x, w, bias, act=0, aux=None, resid=None, Wt=0):
    """(out, pre-activation) in dtype dt on the CPU"""
    v = F.conv2d(x.to(dt), w.to(dt), None if bias is None else bias.to(dt), padding=1)
    pre = v
    if act == 1:
        v = F.gelu(v)
    elif act == 2:
        v = v * _gelu_grad(aux.to(dt))
    if resid is not None:
        v = v + resid.to(dt)
    if Wt:
        v = v.clone()
        v[..., Wt:] = 0.0
    return v, pre


def _run(variant, ncu, x_d, w_d, bias_d, act=0, aux_d=None, resid_d=None, in_place=False, want_pre=False, want_amax=False,
         Wt=0):
    """One launch; returns (out, out_pre or None, amax_out [B] or None) on the CPU."""
    L, lib = _lib()
    B, ci, H, W = x_d.shape
    co = w_d.shape[0]
    nbytes = lib.sinddm_debug_conv_wh_scratch_bytes(ci, co, B)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = resid_d.clone() if in_place else torch.full((B, co, H, W), float("nan"), device=DEV)
    resid = out if in_place else resid_d
    pre = torch.full((B, co, H, W), float("nan"), device=DEV) if want_pre else None
    amax = torch.zeros(B, 8, device=DEV) if want_amax else None
    rc = lib.sinddm_debug_conv_wh(variant, ncu, B, H, W, Wt, ci, co, act, L.ptr(x_d), L.ptr(w_d), L.ptr(bias_d), L.ptr(resid),
                                  L.ptr(aux_d), L.ptr(out), L.ptr(pre), L.ptr(amax), scratch.data_ptr(), nbytes,
                                  L.stream_ptr(DEV))
    L.check(rc, "sinddm_debug_conv_wh")
    torch.cuda.synchronize(DEV)
    return out.cpu(), None if pre is None else pre.cpu(), None if amax is None else amax[:, 0].cpu()


def _errors(got, ref64):
    """per sample: (rel-L2, max-abs) against float64"""
    d = got.double() - ref64
    B = got.shape[0]
    return [(float(d[b].norm() / ref64[b].norm().clamp_min(1e-300)), float(d[b].abs().max())) for b in range(B)]


def _gate(label, got2, got1, ref32, ref64):
    e2, e1, e32 = _errors(got2, ref64), _errors(got1, ref64), _errors(ref32, ref64)
    assert torch.isfinite(got2).all(), label
    for b in range(got2.shape[0]):
        for k, what in enumerate(("rel-L2", "max-abs")):
            yard = max(e1[b][k], e32[b][k])
            print(f"[conv_wr] {label} sample {b} {what}: 160-channel {e2[b][k]:.3e}  80-channel {e1[b][k]:.3e}  fp32 conv2d "
                  f"{e32[b][k]:.3e}  ratio {e2[b][k] / yard:.3f}")
    for b in range(got2.shape[0]):
        for k, what in enumerate(("rel-L2", "max-abs")):
            assert e2[b][k] <= FACTOR * max(e1[b][k], e32[b][k]), (label, b, what, e2[b], e1[b], e32[b])


@pytest.mark.parametrize("co", [160, 320])
@pytest.mark.parametrize("ci", [32, 48, 160])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_against_float64(B, H, W, ci, co):
    x, w, bias = _inputs(B, H, W, ci, co, 3000 + 7 * H + ci + co)
    ref64, _ = _reference(torch.float64, x, w, bias)
    ref32, _ = _reference(torch.float32, x, w, bias)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), bias.to(DEV)
    got2, _, _ = _run(2, 0, x_d, w_d, b_d)
    got1, _, _ = _run(1, 0, x_d, w_d, b_d)
    _gate(f"{B}x{H}x{W} {ci}->{co}", got2, got1, ref32, ref64)
    # the library's choice is the 160-channel kernel; a second call repeats the first
    got0, _, _ = _run(0, 0, x_d, w_d, b_d)
    assert torch.equal(got0, got2)
    assert torch.equal(_run(2, 0, x_d, w_d, b_d)[0], got2)


def test_grids_of_8_and_256_compute_units_agree():
    B, H, W, ci, co = 3, 24, 64, 48, 320
    x, w, bias = _inputs(B, H, W, ci, co, 3100)
    resid = hash_randn((B, co, H, W), 3103)
    ref64, _ = _reference(torch.float64, x, w, bias, resid=resid)
    ref32, _ = _reference(torch.float32, x, w, bias, resid=resid)
    x_d, w_d, b_d, r_d = x.to(DEV), w.to(DEV), bias.to(DEV), resid.to(DEV)
    got = {ncu: _run(2, ncu, x_d, w_d, b_d, resid_d=r_d, in_place=True)[0] for ncu in (8, 256, 0)}
    assert torch.equal(got[8], got[256]) and torch.equal(got[8], got[0])
    assert torch.equal(_run(2, 8, x_d, w_d, b_d, resid_d=r_d, in_place=True)[0], got[8])
    _gate("ncu 8", got[8], _run(1, 8, x_d, w_d, b_d, resid_d=r_d, in_place=True)[0], ref32, ref64)


def test_channel_gains_spanning_2e12():
    B, H, W, ci, co = 2, 9, 36, 48, 160
    x, w, bias = _inputs(B, H, W, ci, co, 3200, gains=True)
    ref64, _ = _reference(torch.float64, x, w, bias)
    ref32, _ = _reference(torch.float32, x, w, bias)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), bias.to(DEV)
    _gate("gains 2^+-6", _run(2, 0, x_d, w_d, b_d)[0], _run(1, 0, x_d, w_d, b_d)[0], ref32, ref64)


def test_library_choice_keeps_the_80_channel_kernel_elsewhere():
    B, H, W, ci, co = 2, 9, 36, 48, 240
    x, w, bias = _inputs(B, H, W, ci, co, 3300)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), bias.to(DEV)
    got1 = _run(1, 0, x_d, w_d, b_d)[0]
    assert torch.equal(_run(0, 0, x_d, w_d, b_d)[0], got1)
    assert torch.isfinite(got1).all()


@pytest.mark.parametrize("option", ["act0", "act1", "act2", "out_pre", "resid_in_place", "no_bias", "Wt34", "amax_out"])
def test_epilogue_options(option):
    B, H, W, ci, co = 2, 9, 36, 48, 160
    Wt = 34 if option == "Wt34" else 0
    x, w, bias = _inputs(B, H, W, ci, co, 3400, Wt=Wt)
    act = {"act1": 1, "act2": 2, "out_pre": 1}.get(option, 0)
    aux = hash_randn((B, co, H, W), 3404) if act == 2 else None
    resid = hash_randn((B, co, H, W), 3405) if option == "resid_in_place" else None
    if option == "no_bias":
        bias = None
    ref64, pre64 = _reference(torch.float64, x, w, bias, act, aux, resid, Wt)
    ref32, pre32 = _reference(torch.float32, x, w, bias, act, aux, resid, Wt)
    dev = lambda t: None if t is None else t.to(DEV)
    kw = dict(act=act, aux_d=dev(aux), resid_d=dev(resid), in_place=resid is not None, want_pre=option == "out_pre",
              want_amax=option == "amax_out", Wt=Wt)
    got2, pre2, amax2 = _run(2, 0, x.to(DEV), w.to(DEV), dev(bias), **kw)
    got1, pre1, _ = _run(1, 0, x.to(DEV), w.to(DEV), dev(bias), **kw)
    _gate(option, got2, got1, ref32, ref64)
    if option == "out_pre":
        _gate("out_pre (pre-activation)", pre2, pre1, pre32, pre64)
    if option == "Wt34":
        assert (got2[..., Wt:] == 0).all()
    if option == "amax_out":
        assert torch.equal(amax2, got2.abs().amax(dim=(1, 2, 3)))
