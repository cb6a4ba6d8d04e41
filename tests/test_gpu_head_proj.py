"""GPU: the head's projection formed in conv_wr_kernel's epilogue (csrc/conv_wh.h, ConvArgs::proj_w / proj_out), ONE LAUNCH
AT A TIME through sinddm_debug_conv_wr_proj, and one network evaluation that uses it.

Kernel level.  proj_out[b][o][y][x] = sum_co proj_w[co][o] * out[b][co][y][x] over the fp32 values the kernel itself stores:
  shapes    (1, 8, 32) one exact item, (2, 9, 36) partial tiles on both axes, (3, 17, 68) with true width 66 (pad columns);
  channels  C_in 32 (the two-chunk minimum) and 160, C_out 160;
  residual  absent, a separate tensor, `out` itself.
  accuracy  against the float64 sum of the kernel's own fp32 output every element satisfies
            |err| <= (160 + 4) 2^-24 sum_co |proj_w[co][o] out[co]|:  the sum is 10 fmas per 16-channel partial, then 15 adds
            of the partials -- at most 25 roundings on any path, each relative to a partial sum that the absolute sum
            bounds; 160 + 4 is the bound of a 160-term sum in ANY order, so the test holds the kernel to the rounding model
            and not to its present order;
  extent    pad columns of proj_out are zeros, nothing is written behind the last row (a NaN guard band stays NaN);
  bits      `out` is the same with and without the projection and equals sinddm_debug_conv_wh's variant 2; grids of 8 and
            256 compute units give the same `out` and proj_out; a second call repeats the first.

End to end.  sinddm_net_forward at 16 x 186 x 248, dim 160 -- the smallest C2 shape whose plan hands block 3's conv2 to
conv_wr_kernel on 256 compute units -- with He-normal weights, against the same call under SINDDM_DIM_HEAD_XIN.  The two
differ by the rounding of one 160-term sum in two orders: a priori |diff| <= 160 2^-24 sum_c |W_r[o][c] x_in[c]| each way,
asserted against twice that.  The batch holds two distinct samples eight times over (the float32 evaluation of blocks 1-3
that yields x_in for the bound then costs two samples on the CPU); copies must agree bit for bit.
reference SinDDM/models.py:79-80 (the residual projection), :132,150 (final_conv)"""
import math

import pytest
import torch

from sinddm_amd.synth import hash_randn, he_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
CO = 160
SHAPES = [(1, 8, 32, 0), (2, 9, 36, 0), (3, 17, 68, 66)]
GUARD = 1024


def _lib():
    from sinddm_amd import _lib
    return _lib, _lib.load()


_IN = {}


def _inputs(B, H, W, Wt, ci):
    """x, weights, bias, residual, projection weights: made once per (shape, C_in), never changed"""
    key = (B, H, W, Wt, ci)
    if key not in _IN:
        seed = 4200 + 11 * H + ci
        x = hash_randn((B, ci, H, W), seed)
        w = hash_randn((CO, ci, 3, 3), seed + 1) * math.sqrt(2.0 / (9 * ci))
        bias = hash_randn((CO,), seed + 2) * 0.1
        resid = hash_randn((B, CO, H, W), seed + 3)
        pw = hash_randn((CO, 3), seed + 4) * math.sqrt(1.0 / CO)
        if Wt:
            x[..., Wt:] = 0.0
            resid[..., Wt:] = 0.0
        _IN[key] = tuple(t.to(DEV) for t in (x, w, bias, resid, pw))
    return _IN[key]


def _run(ncu, x_d, w_d, b_d, pw_d, resid_mode, resid_d, Wt, proj=True):
    """One launch of sinddm_debug_conv_wr_proj; returns (out, proj_out with its guard band or None) on the device."""
    L, lib = _lib()
    B, ci, H, W = x_d.shape
    nbytes = lib.sinddm_debug_conv_wh_scratch_bytes(ci, CO, B)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    if resid_mode == "aliased":
        out = resid_d.clone()
        resid = out
    else:
        out = torch.full((B, CO, H, W), float("nan"), device=DEV)
        resid = resid_d if resid_mode == "separate" else None
    pbuf = torch.full((B * 3 * H * W + GUARD,), float("nan"), device=DEV) if proj else None
    rc = lib.sinddm_debug_conv_wr_proj(ncu, B, H, W, Wt, ci, CO, L.ptr(x_d), L.ptr(w_d), L.ptr(b_d), L.ptr(resid),
                                       L.ptr(pw_d) if proj else None, L.ptr(out), L.ptr(pbuf), scratch.data_ptr(), nbytes,
                                       L.stream_ptr(DEV))
    L.check(rc, "sinddm_debug_conv_wr_proj")
    torch.cuda.synchronize(DEV)
    return out, pbuf


def _plain_variant2(x_d, w_d, b_d, resid_mode, resid_d, Wt):
    L, lib = _lib()
    B, ci, H, W = x_d.shape
    nbytes = lib.sinddm_debug_conv_wh_scratch_bytes(ci, CO, B)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = resid_d.clone() if resid_mode == "aliased" else torch.full((B, CO, H, W), float("nan"), device=DEV)
    resid = out if resid_mode == "aliased" else resid_d if resid_mode == "separate" else None
    rc = lib.sinddm_debug_conv_wh(2, 0, B, H, W, Wt, ci, CO, 0, L.ptr(x_d), L.ptr(w_d), L.ptr(b_d), L.ptr(resid), None,
                                  L.ptr(out), None, None, scratch.data_ptr(), nbytes, L.stream_ptr(DEV))
    L.check(rc, "sinddm_debug_conv_wh")
    torch.cuda.synchronize(DEV)
    return out


@pytest.mark.parametrize("resid_mode", ["absent", "separate", "aliased"])
@pytest.mark.parametrize("ci", [32, 160])
@pytest.mark.parametrize("B,H,W,Wt", SHAPES)
def test_projection_of_the_kernels_own_output(B, H, W, Wt, ci, resid_mode):
    x_d, w_d, b_d, r_d, pw_d = _inputs(B, H, W, Wt, ci)
    out, pbuf = _run(0, x_d, w_d, b_d, pw_d, resid_mode, r_d, Wt)
    n = B * 3 * H * W
    proj = pbuf[:n].view(B, 3, H, W)
    assert torch.isfinite(out).all() and torch.isfinite(proj).all()
    # nothing behind the last row of the last plane
    assert torch.isnan(pbuf[n:]).all()
    # accuracy: float64 sum of the kernel's own fp32 output
    o64, p64 = out.double().cpu(), pw_d.double().cpu()
    ref = torch.einsum("co,bchw->bohw", p64, o64)
    mag = torch.einsum("co,bchw->bohw", p64.abs(), o64.abs())
    err = (proj.double().cpu() - ref).abs()
    bound = (CO + 4) * U * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"[head_proj] {B}x{H}x{W} Wt {Wt} C_in {ci} resid {resid_mode}: max |err| {float(err.max()):.3e}, "
          f"max |err| / bound {worst:.4f}, max bound {float(bound.max()):.3e}")
    assert (err <= bound).all(), (worst, float(err.max()))
    # pad columns: zeros in `out` and in the projection
    if Wt:
        assert (out[..., Wt:] == 0).all() and (proj[..., Wt:] == 0).all()
    # `out` does not know about the projection
    out_plain, _ = _run(0, x_d, w_d, b_d, pw_d, resid_mode, r_d, Wt, proj=False)
    assert torch.equal(out_plain, out)
    assert torch.equal(_plain_variant2(x_d, w_d, b_d, resid_mode, r_d, Wt), out)
    # grids of 8 and 256 compute units, and a second call
    for ncu in (8, 256, 0):
        o2, p2 = _run(ncu, x_d, w_d, b_d, pw_d, resid_mode, r_d, Wt)
        assert torch.equal(o2, out), ncu
        assert torch.equal(p2[:n], pbuf[:n]) and torch.isnan(p2[n:]).all(), ncu


def test_hook_refuses_what_the_kernel_cannot_do():
    L, lib = _lib()
    B, H, W, ci = 1, 8, 32, 32
    x_d, w_d, b_d, r_d, pw_d = _inputs(B, H, W, 0, ci)
    nbytes = lib.sinddm_debug_conv_wh_scratch_bytes(ci, 320, B)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.zeros(B, 320, H, W, device=DEV)
    pr = torch.zeros(B, 3, H, W, device=DEV)
    args = lambda co, pw, po: (0, B, H, W, 0, ci, co, L.ptr(x_d), L.ptr(w_d), L.ptr(b_d), None, pw, L.ptr(out), po,
                               scratch.data_ptr(), nbytes, L.stream_ptr(DEV))
    assert lib.sinddm_debug_conv_wr_proj(*args(320, L.ptr(pw_d), L.ptr(pr))) == -2     # an item holds half the channels
    assert lib.sinddm_debug_conv_wr_proj(*args(80, L.ptr(pw_d), L.ptr(pr))) == -2
    assert lib.sinddm_debug_conv_wr_proj(*args(CO, None, L.ptr(pr))) == -1             # a projection without weights
    assert lib.sinddm_debug_conv_wr_proj(*args(CO, L.ptr(pw_d), pr.data_ptr() + 4)) == -1   # 16-byte stores
    torch.cuda.synchronize(DEV)
    assert (pr == 0).all()


def test_network_forward_agrees_with_the_x_in_head():
    import ctypes as C
    from oracle import sinddm_oracle as O
    from sinddm_amd.models import SinDDMNet
    L, lib = _lib()
    dim, B, H, W, scale = 160, 16, 186, 248, 4
    ext2 = 85
    flags = (C.c_int64 * ext2)()
    assert lib.sinddm_debug_forward_plan(dim, 0, B, H, W, 0, flags, ext2) == 0
    ncu = int(flags[23])
    if ncu < 256:
        assert flags[84] in (0, 1)
    else:
        assert flags[84] == 1, "this shape must take the projected head on a device of 256 compute units"
    assert lib.sinddm_debug_forward_plan(dim | L.DIM_HEAD_XIN, 0, B, H, W, 0, flags, ext2) == 0 and flags[84] == 0

    sd = he_state_dict(dim)
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    net.load_state_dict(sd)
    x2 = hash_randn((2, 3, H, W), 4300)
    t2 = torch.tensor([17, 503])
    x = x2.repeat(B // 2, 1, 1, 1).to(DEV)            # sample b = sample b % 2
    t = t2.repeat(B // 2).to(DEV)
    with torch.no_grad():
        net.head_xin = False
        got = net(x, t, scale=scale).clone()
        again = net(x, t, scale=scale).clone()
        net.head_xin = True
        xin_form = net(x, t, scale=scale).clone()
        net.head_xin = False
    torch.cuda.synchronize(DEV)
    assert torch.isfinite(got).all() and torch.equal(got, again)
    for b in range(2, B):
        assert torch.equal(got[b], got[b % 2]), b        # the order of the sums is the item's own, whatever its sample

    # the a-priori bound: x_in = block 3's output (float32 on the CPU: only its magnitude matters), W_r composed in float64
    cond = O.cond_vector(sd, t2, scale)
    h = x2
    for name in ("l1", "l2", "l3"):
        h = O.conv_block(sd, name, h, cond)
    wr = sd["final_conv.0.weight"].double().view(3, dim // 2) @ sd["l4.res_conv.weight"].double().view(dim // 2, dim)
    mag = torch.einsum("oc,bchw->bohw", wr.abs(), h.double().abs())
    bound = 2.0 * CO * U * mag
    diff = (got[:2].double().cpu() - xin_form[:2].double().cpu()).abs()
    print(f"[head_proj] net forward {B}x{H}x{W} dim {dim}: max |projected - x_in form| {float(diff.max()):.3e}, "
          f"max over elements of |diff| / (160 2^-24 sum |W_r x|) {float((diff / (bound / 2).clamp_min(1e-300)).max()):.4f}, "
          f"rel-L2 {float(diff.norm() / xin_form[:2].double().cpu().norm()):.3e}")
    assert (diff <= bound).all()
    assert float(diff.max()) > 0.0 or ncu < 256      # two summation orders: not the same kernel twice
