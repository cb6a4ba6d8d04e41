"""The depthwise 5x5 rows kernel (dwconv5_rows_kernel) and the first 3x3 conv (conv3x3_c3_gelu_kernel), element by element.

One block's forward through sinddm_debug_block_train.  The call returns only the block's output, so the depthwise output h
and the first conv's pre-activation u and GELU g are read from the training workspace the test itself supplies: the layout
below mirrors carve_train (sinddm_bwd.hip), and the mirror is checked on every call (the block's output region must equal the
returned y bit for bit).

Depthwise, block 2 of dim 160 (80 channels), hash noise, against a float64 F.conv2d:
    |err| <= 27 * 2^-24 * (|w| (*) |x| + |bias| + |cond|)        the standard bound of a 26-term fp32 sum
at (B, H, W) = (1, 1, 192) one 256-column band whose last lanes are outside the image, fewer rows than a wave owns;
(2, 13, 256) one full band; (1, 49, 260) two bands, the second with one live lane, a wave whose first row is the image's last;
(2, 50, 516) three bands; (1, 65, 260) one row more than the 64 of a workgroup's four waves.  Every quad differs from both of its neighbours (asserted), so a lane that took its outer columns
from the wrong neighbour lane cannot pass.  Padded rows (W % 4 != 0, W >= 192: the kernel writes the pad columns as zeros and
the aligned kernels behind it read them unmasked) go through sinddm_net_forward on He weights, judged like
tests/test_gpu_fullrank.py: 3 x the error of the fp32 oracle against float64, whole tensor and edge regions.

First conv (block 1's 3 -> dim/2 conv + GELU), input = the depthwise output the library itself wrote, against a float64
F.gelu(F.conv2d(...)):
    |err| <= 29 * 2^-24 * (|w| (*) |x| + |b|)                    on the pre-activation (a 28-term fp32 sum), and
    |err| <= 29 * 2^-24 * (|w| (*) |x| + |b|) + 1.7e-6           on the GELU (its slope is at most 1.13, so the linear bound
                                                                  carries through; 1.7e-6 is the absolute error common.h
                                                                  documents for gelu_erf2)
at 5x8 (smaller than a tile), 16x20 (a row end inside a pixel group), 33x260 (several workgroups); dim 160, and dim 20 for the
channel-split launch.                                 reference SinDDM/models.py:51-80
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import max_abs, rel_l2
from fullrank_util import edge_regions, net_forward_f64
from oracle import sinddm_oracle as O
from sinddm_amd.synth import hash_randn, he_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_SD, _NETS = {}, {}


def _lib():
    from sinddm_amd import _lib
    return _lib, _lib.load()


def _net(dim):
    if dim not in _NETS:
        from sinddm_amd.models import SinDDMNet
        _SD[dim] = he_state_dict(dim)
        net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
        net.load_state_dict(_SD[dim])
        _NETS[dim] = net
    return _NETS[dim], _SD[dim]


def _train_layout(lib, dim, B, H, W):
    """Byte offsets of h / u / g / o of each block inside the training workspace (carve_train: every region rounded up to 256 B)."""
    au = lambda nfloats: (nfloats * 4 + 255) // 256 * 256
    off = au(B * lib.sinddm_cond_stride(dim)) + au(B * 64) + au(B * 128) + au(B * 32) + au(B * 128)
    out = []
    for cin, cout in O.block_channels(dim):
        d = {}
        for name, ch in (("h", cin), ("u", cout), ("g", cout), ("o", cout)):
            d[name] = off
            off += au(B * ch * H * W)
        out.append(d)
    return out


def _block_forward(dim, li, x, cb):
    """Block `li` on x with the per-sample condition cb: {h, u, g} from the workspace (CPU tensors)."""
    L, lib = _lib()
    net, _ = _net(dim)
    B, cin, H, W = x.shape
    cout = O.block_channels(dim)[li][1]
    ws = torch.zeros(int(lib.sinddm_train_workspace_bytes(dim, B, H, W)), dtype=torch.uint8, device=DEV)
    y = torch.empty(B, cout, H, W, device=DEV)
    gx = torch.empty(B, cin, H, W, device=DEV)
    dc = torch.zeros(B, cin, device=DEV)
    gr = torch.zeros_like(net.flat_params)
    xd, cbd, gyd = x.to(DEV), cb.to(DEV), torch.zeros(B, cout, H, W, device=DEV)
    L.check(lib.sinddm_debug_block_train(L.ptr(net.flat_params), L.ptr(net.packed_weights()), L.ptr(net.packed_weights_bwd()),
                                         dim, li, L.ptr(xd), L.ptr(cbd), L.ptr(gyd), L.ptr(y), L.ptr(gx), L.ptr(gr), L.ptr(dc),
                                         B, H, W, ws.data_ptr(), ws.numel(), L.stream_ptr(DEV)), "sinddm_debug_block_train")
    torch.cuda.synchronize()
    lay = _train_layout(lib, dim, B, H, W)[li]

    def region(name, ch):
        n = B * ch * H * W
        return ws[lay[name]:lay[name] + 4 * n].view(torch.float32).reshape(B, ch, H, W).cpu()
    assert torch.equal(region("o", cout), y.cpu()), "the workspace layout mirrored here is not carve_train's"
    return {"h": region("h", cin), "u": region("u", cout), "g": region("g", cout)}


DW_SHAPES = [(1, 1, 192), (2, 13, 256), (1, 49, 260), (2, 50, 516), (1, 65, 260)]


@pytest.mark.parametrize("B,H,W", DW_SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in DW_SHAPES])
def test_depthwise_rows_block2_elementwise_vs_float64(B, H, W):
    dim, li = 160, 1
    _, sd = _net(dim)
    cin = O.block_channels(dim)[li][0]
    assert cin == 80 and W % 4 == 0 and W >= 192                        # the rows kernel's launch rule (dwconv_launch)
    x = hash_randn((B, cin, H, W), 900 + W)
    cb = 0.5 * hash_randn((B, cin), 901 + W)
    q = x.reshape(B, cin, H, W // 4, 4)
    assert bool((q[..., 1:, :] != q[..., :-1, :]).any(-1).all()), "two neighbouring quads are equal"
    got = _block_forward(dim, li, x, cb)["h"].double()
    w, b = sd["l2.ds_conv.weight"].double(), sd["l2.ds_conv.bias"].double()
    ref = F.conv2d(x.double(), w, b, padding=2, groups=cin) + cb.double()[:, :, None, None]
    mag = F.conv2d(x.double().abs(), w.abs(), b.abs(), padding=2, groups=cin) + cb.double().abs()[:, :, None, None]
    ratio = ((got - ref).abs() / (27 * 2.0 ** -24 * mag)).max().item()
    print(f"[dw rows {B}x{H}x{W}] max |err| / bound = {ratio:.3f}; max |err| {max_abs(got, ref):.3e}")
    assert ratio <= 1.0


def test_depthwise_rows_padded_rows_net_forward_vs_float64():
    """W % 4 = 2, padded to 196 >= 192: every depthwise launch of the forward is the rows kernel with Wt < W."""
    dim, B, H, W = 160, 1, 6, 194
    L, lib = _lib()
    assert lib.sinddm_debug_head_path(dim, B, H, W) == 1               # (the plan pads its rows)
    net, sd = _net(dim)
    x = hash_randn((B, 3, H, W), 77) * 0.9
    t = torch.tensor([417], dtype=torch.long)
    with torch.no_grad():
        ref64, ref32 = net_forward_f64(sd, x, t, 2), O.net_forward(sd, x, t, 2)
    got = net.infer(x.to(DEV), t.to(DEV), 0, 2.0).cpu()
    assert torch.isfinite(got).all()
    e_k, e_32 = rel_l2(got, ref64), rel_l2(ref32, ref64)
    line, fails = f"[dw rows padded {B}x{H}x{W}] rel-L2 vs float64: library {e_k:.3e} fp32 oracle {e_32:.3e}", []
    if e_k > 3 * e_32:
        fails.append(("rel_l2", e_k, e_32))
    for name, m in edge_regions(H, W):
        a_k, a_32 = max_abs(got[..., m], ref64[..., m]), max_abs(ref32[..., m], ref64[..., m])
        line += f"; {name} max-abs {a_k:.3e} vs {a_32:.3e}"
        if a_k > 6 * a_32:
            fails.append((name, a_k, a_32))
    print(line)
    assert not fails, fails


C3_SHAPES = [(5, 8), (16, 20), (33, 260)]


@pytest.mark.parametrize("dim", [160, 20])
@pytest.mark.parametrize("H,W", C3_SHAPES, ids=[f"{h}x{w}" for h, w in C3_SHAPES])
def test_first_conv_gelu_elementwise_vs_float64(dim, H, W):
    li, B = 0, 2
    _, sd = _net(dim)
    x = hash_randn((B, 3, H, W), 300 + W)
    cb = 0.5 * hash_randn((B, 3), 301 + W)
    got = _block_forward(dim, li, x, cb)
    h = got["h"].double()                                              # the conv's input as the library wrote it
    w, b = sd["l1.net.0.weight"].double(), sd["l1.net.0.bias"].double()
    pre = F.conv2d(h, w, b, padding=1)
    mag = F.conv2d(h.abs(), w.abs(), b.abs(), padding=1)
    lin = 29 * 2.0 ** -24 * mag
    r_u = ((got["u"].double() - pre).abs() / lin).max().item()
    r_g = ((got["g"].double() - F.gelu(pre)).abs() / (lin + 1.7e-6)).max().item()
    print(f"[first conv dim {dim} {H}x{W}] max |err| / bound: pre-activation {r_u:.3f}, GELU {r_g:.3f}")
    assert r_u <= 1.0 and r_g <= 1.0
