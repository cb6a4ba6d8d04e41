"""GPU: the collapsed inference head (csrc/head.h).  In inference block 4's conv2, its residual projection and final_conv
run as ONE kernel, eps = conv3x3(g; W_c) + conv1x1(x_in; W_r) + b_c, on weights composed when the packed image is built.

  H1  the composed weights in the packed image are the float64 composition rounded to fp32, to one ulp;
  H2  the head's kernel alone (sinddm_debug_head) on hash noise is NOT wider than the uncollapsed head evaluated in fp32
      (torch CPU: conv2, projection, add, final conv), measured against that same head in float64 -- in rel-L2, and in
      max-abs on the one-pixel border ring and on the interior separately, so that a padding error cannot hide in a norm;
  H3  the whole inference forward keeps the project's gates (tests/test_gpu_h2.py) on both conv settings, at shapes that
      take the head and at one that keeps the old launches; every case asserts which of the two it ran;
  H4  the fused chain and the step-by-step route share the head: they agree within the bound of tests/test_gpu_seeds.py,
      plain and with ROI + keep maps + per-sample seeds; one and two streams are bit-equal.
reference SinDDM/models.py:69-80 (the block), :130-132,151 (final_conv), :449-459 (the step)
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import max_abs, rel_l2
from fullrank_util import net_forward_f64 as _net_forward_f64
from oracle import sinddm_oracle as O
from sinddm_amd.synth import closed_form_state_dict, hash_randn
from test_head_host import compose_head

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from sinddm_amd import _lib
    return _lib, _lib.load()


_NETS = {}


def _net(dim):
    """One network per width for the whole module (closed-form weights; nothing here changes them)."""
    if dim not in _NETS:
        from sinddm_amd.models import SinDDMNet
        net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
        net.load_state_dict(closed_form_state_dict(dim))
        _NETS[dim] = net
    return _NETS[dim]


# ---- H1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 160])
def test_composed_weights_in_the_packed_image(dim):
    _check_composed_weights(dim, _net(dim), closed_form_state_dict(dim))


def _check_composed_weights(dim, net, sd):
    """H1 on the network `net` loaded with the state dict `sd` (tests/test_gpu_fullrank.py runs it on He weights)."""
    L, lib = _lib()
    half = dim // 2
    packed = net.packed_weights()
    torch.cuda.synchronize()
    off = (C.c_int64 * 3)()
    assert lib.sinddm_debug_head_offsets(dim, off) == 0
    assert off[2] + 3 == packed.numel() == lib.sinddm_packed_count(dim)
    img = packed.cpu().numpy()
    wc, wr, bc = compose_head(sd)
    want = [wc.permute(1, 0, 2, 3).reshape(-1),                              # [ci][o][tap]
            wr[:, :, 0, 0].t().reshape(-1),                                  # [ci][o]
            bc]
    for name, o, w64 in zip(("W_c", "W_r", "b_c"), off, want):
        w32 = w64.float().numpy()
        got = img[o:o + w32.size]
        ulps = np.abs(got.astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)
        print(f"dim {dim} {name}: {w32.size} elements, worst {float(ulps.max()):.2f} ulp, {int((got != w32).sum())} differ")
        assert float(ulps.max()) <= 1.0, name
        assert float(np.abs(w32).max()) > 0


# ---- H2 ----------------------------------------------------------------------------------------------------------------------
# (H, W, pitch): 1x4 = one quad, no neighbours, H = 1; 13x17 on padded rows; 33x36 = 297 quads per sample: a block boundary
# falls inside a sample
HEAD_SHAPES = [(1, 4, 4), (5, 8, 8), (9, 12, 12), (13, 17, 20), (33, 36, 36)]


@pytest.mark.parametrize("H,W,Wp", HEAD_SHAPES, ids=[f"{h}x{w}_pitch{p}" for h, w, p in HEAD_SHAPES])
@pytest.mark.parametrize("dim", [160, 32])
def test_head_alone_is_not_wider_than_the_uncollapsed_head_in_fp32(dim, H, W, Wp):
    _check_head_alone(dim, H, W, Wp, _net(dim), closed_form_state_dict(dim))


def _check_head_alone(dim, H, W, Wp, net, sd):
    """H2 on the network `net` loaded with the state dict `sd` (tests/test_gpu_fullrank.py runs it on He weights)."""
    L, lib = _lib()
    B, half = 3, dim // 2
    g = hash_randn((B, half, H, W), 900 + H)
    x_in = hash_randn((B, dim, H, W), 901 + W)

    def uncollapsed(dt):
        s = {k: v.to(dt) for k, v in sd.items()}
        o = F.conv2d(g.to(dt), s["l4.net.2.weight"], s["l4.net.2.bias"], padding=1)
        r = F.conv2d(x_in.to(dt), s["l4.res_conv.weight"], s["l4.res_conv.bias"])
        return F.conv2d(o + r, s["final_conv.0.weight"], s["final_conv.0.bias"])

    ref64, ref32 = uncollapsed(torch.float64), uncollapsed(torch.float32)
    gp, xp = torch.zeros(B, half, H, Wp), torch.zeros(B, dim, H, Wp)          # padded rows, pad columns zero
    gp[..., :W], xp[..., :W] = g, x_in
    gp, xp = gp.to(DEV), xp.to(DEV)
    got = torch.full((B, 3, H, W), float("nan"), device=DEV)
    L.check(lib.sinddm_debug_head(L.ptr(net.packed_weights()), L.ptr(gp), L.ptr(xp), L.ptr(got), dim, B, H, W, Wp,
                                  L.stream_ptr(DEV)), "sinddm_debug_head")
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.isfinite(got).all()
    e_k, e_32 = rel_l2(got, ref64), rel_l2(ref32, ref64)
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    parts = [("ring", ring)] + ([("interior", ~ring)] if bool((~ring).any()) else [])
    line = f"dim {dim} {H}x{W} pitch {Wp}: vs float64 rel-L2 head {e_k:.3e} fp32 uncollapsed {e_32:.3e} (ratio {e_k / e_32:.2f})"
    worst = []
    for name, m in parts:
        a_k, a_32 = max_abs(got[..., m], ref64[..., m]), max_abs(ref32[..., m], ref64[..., m])
        line += f"; {name} max-abs {a_k:.3e} vs {a_32:.3e}"
        worst.append((name, a_k, a_32))
    print(line)
    assert e_k <= e_32, (e_k, e_32)
    for name, a_k, a_32 in worst:
        assert a_k <= 2 * a_32, (name, a_k, a_32)


def test_head_arguments():
    L, lib = _lib()
    t = torch.zeros(64, device=DEV)
    p = L.ptr(t)
    assert lib.sinddm_debug_head(p, p, p, p, 160, 1, 4, 6, 6, None) == -2     # pitch not a multiple of 4
    assert lib.sinddm_debug_head(p, p, p, p, 160, 1, 4, 4, 12, None) == -2    # more than a quad of padding
    assert lib.sinddm_debug_head(p, p, p, p, 160, 1, 4, 9, 8, None) == -2     # rows wider than their pitch
    assert lib.sinddm_debug_head(p, p, p, p, 3, 1, 4, 8, 8, None) == -2


# ---- H3 ----------------------------------------------------------------------------------------------------------------------
FWD = [(160, 2, 13, 17, 1), (160, 2, 33, 36, 1), (160, 1, 8, 16, 1), (32, 2, 9, 12, 1), (20, 2, 9, 12, 1), (20, 2, 9, 13, 0)]
_REFS = {}


def _refs(dim, B, H, W):
    key = (dim, B, H, W)
    if key not in _REFS:
        sd = closed_form_state_dict(dim)
        x = hash_randn((B, 3, H, W), 1234 + W) * 0.9
        t = torch.tensor([(53 * (i + 3)) % 1000 for i in range(B)], dtype=torch.long)
        _REFS[key] = (x, t, _net_forward_f64(sd, x, t, 2), O.net_forward(sd, x, t, 2))
    return _REFS[key]


@pytest.mark.parametrize("fp32_convs", [False, True], ids=["default_convs", "fp32_convs"])
@pytest.mark.parametrize("dim,B,H,W,path", FWD, ids=[f"dim{d}_{b}x{h}x{w}_head{p}" for d, b, h, w, p in FWD])
def test_inference_forward_keeps_the_gates(dim, B, H, W, path, fp32_convs):
    L, lib = _lib()
    net = _net(dim)
    assert lib.sinddm_debug_head_path(dim | (L.DIM_FP32_CONVS if fp32_convs else 0), B, H, W) == path
    x, t, ref64, ref32 = _refs(dim, B, H, W)
    net.fp32_convs = fp32_convs
    try:
        got = net.infer(x.to(DEV), t.to(DEV), 0, 2.0).cpu()
    finally:
        net.fp32_convs = False
    assert torch.isfinite(got).all()
    e_k, e_32, e_o = rel_l2(got, ref64), rel_l2(ref32, ref64), rel_l2(got, ref32)
    print(f"dim {dim} {B}x{H}x{W} head_path {path} fp32_convs {fp32_convs}: vs float64 library {e_k:.3e} fp32 oracle {e_32:.3e}; "
          f"library vs fp32 oracle {e_o:.3e}")
    assert e_o < 1e-5
    assert e_k <= 1.5 * e_32, (e_k, e_32)


# ---- H4 ----------------------------------------------------------------------------------------------------------------------
def _fill(n, seed, stream):
    L, lib = _lib()
    out = torch.empty(n, device=DEV)
    L.check(lib.sinddm_normal_fill(L.ptr(out), n, seed, stream, L.stream_ptr(DEV)), "sinddm_normal_fill")
    return out


def _chain(net, d, s, x0, xt, ts, seed, sid0, aux, edit=None, keep=None, seeds=None):
    """sinddm_sample_chain_seeds (every option the chain has; NULL for the ones not given)."""
    from sinddm_amd.models import _aux_stream, _workspace
    L, lib = _lib()
    B, _, H, W = x0.shape
    n = len(ts)
    xa, xb, eps = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
    tab = d._coef_table(s)
    coefs = (L.StepCoefs * n)(*[tab[t] for t in ts])
    tl = (C.c_int * n)(*ts)
    ws = _workspace(DEV, lib.sinddm_workspace_bytes(net.dim, B, H, W))
    flag = C.c_int(-1)
    opts = L.ChainOpts()
    if edit is not None:
        opts.edit_w, opts.edit_c = L.ptr(edit[0]), L.ptr(edit[1])
    kopts = None
    if keep is not None:
        ab_tab = d._keep_ab_table()
        ab = (C.c_float * (2 * n))(*[float(v) for t in ts for v in ab_tab[t]])
        kopts = L.KeepOpts()
        kopts.mask, kopts.x0, kopts.ab = L.ptr(keep[0]), L.ptr(keep[1]), C.cast(ab, C.POINTER(C.c_float))
    sd = torch.tensor(seeds, dtype=torch.int64, device=DEV) if seeds is not None else None
    rc = lib.sinddm_sample_chain_seeds(
        L.ptr(net.flat_params), L.ptr(net.packed_weights()), L.ptr(xa), L.ptr(xb), L.ptr(eps), L.ptr(xt), coefs, tl, n,
        float(s), seed, sid0, net.dim, B, H, W, ws.data_ptr(), ws.numel(), L.stream_ptr(DEV),
        _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, 0,
        C.byref(kopts) if kopts is not None else None, L.ptr(sd))
    torch.cuda.synchronize()
    assert rc == 0 and flag.value in (0, 1)
    return xb if flag.value == 1 else xa


@pytest.mark.parametrize("options", [False, True], ids=["plain", "roi_keep_seeds"])
@pytest.mark.parametrize("H,W", [(13, 17), (16, 16)], ids=["13x17_padded_rows", "16x16_plain_rows"])
def test_fused_chain_equals_stepwise_route(H, W, options):
    """Three steps incl. t = 0 of scale 1 (mode 1: x-tilde is read), dim 160, B = 2: the chain call against
    sinddm_net_forward + sinddm_reverse_step(_keep) per step fed the chain's own draws."""
    from sinddm_amd.configs import build_diffusion
    L, lib = _lib()
    dim, B, s, ts = 160, 2, 1, [400, 1, 0]
    assert lib.sinddm_debug_head_path(dim, B, H, W) == 1
    net, d = build_diffusion("C2", dim=dim, device=DEV)
    x0 = (hash_randn((B, 3, H, W), 41) * 0.8).to(DEV)
    xt = (hash_randn((B, 3, H, W), 42) * 0.5).clamp(-1, 1).to(DEV)
    seed, sid0 = 515152, 7
    seeds = [3, (1 << 63) - 1] if options else None
    edit = keep = None
    if options:
        ew = torch.ones(H, W)
        ew[2:9, 3:11] = 0.2                                                  # (an edge off the quad grid)
        ec = hash_randn((3, H, W), 43) * 0.3 * (1 - ew)
        m = torch.zeros(H, W)
        m[4:, 5:] = 1
        m[6:10, 1:9] = 0.25
        k0 = (hash_randn((3, H, W), 44) * 0.6).clamp(-1, 1)
        edit, keep = (ew.to(DEV), ec.to(DEV).contiguous()), (m.to(DEV), k0.to(DEV))
    tab, ab_tab = d._coef_table(s), d._keep_ab_table()
    n1 = 3 * H * W
    x = x0.clone()
    for i, t in enumerate(ts):
        eps = net.infer(x, None, t, float(s))
        if seeds is not None:
            z = torch.stack([_fill(n1, sd, sid0 + i) for sd in seeds]).view_as(x)
        else:
            z = _fill(x.numel(), seed, sid0 + i).view_as(x)
        out = torch.empty_like(x)
        k = tab[t]
        if options:
            ka, kb = (float(v) for v in ab_tab[t])
            L.check(lib.sinddm_reverse_step_keep(L.ptr(x), L.ptr(eps), L.ptr(xt), L.ptr(z), L.ptr(out), C.byref(k),
                                                 L.ptr(edit[0]), L.ptr(edit[1]), L.ptr(keep[0]), L.ptr(keep[1]), ka, kb, B, 3,
                                                 H * W, L.stream_ptr(DEV)), "sinddm_reverse_step_keep")
        else:
            L.check(lib.sinddm_reverse_step(L.ptr(x), L.ptr(eps), L.ptr(xt), L.ptr(z), L.ptr(out), C.byref(k), x.numel(),
                                            L.stream_ptr(DEV)), "sinddm_reverse_step")
        x = out
    torch.cuda.synchronize()
    y = _chain(net, d, s, x0, xt, ts, seed, sid0, False, edit=edit, keep=keep, seeds=seeds)
    assert torch.isfinite(y).all()
    err, bound = max_abs(y.cpu(), x.cpu()), 4e-6 * max(1.0, float(x.abs().max()))
    y2 = _chain(net, d, s, x0, xt, ts, seed, sid0, True, edit=edit, keep=keep, seeds=seeds)
    print(f"{H}x{W} options={options}: fused chain vs stepwise max-abs {err:.3e} (bound {bound:.3e}); one vs two streams "
          f"bit-equal {torch.equal(y, y2)}")
    assert err <= bound
    assert torch.equal(y, y2)
    assert max_abs(y.cpu(), x0.cpu()) > 1e-2                                 # (the steps did move the sample)
