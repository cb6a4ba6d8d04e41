"""GPU parity tests of the training path: HIP forward-with-save + backward + L1 loss + fused Adam/EMA
(through the C ABI) vs golden fixtures from the reference and vs the CPU oracle's autograd."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import max_abs, rel_l2
from fullrank_util import klass
from oracle import sinddm_oracle as O
from sinddm_amd.synth import closed_form_state_dict, hash_randn, noise_key

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pyr_tensor(arr):
    return torch.from_numpy(arr.transpose(2, 0, 1).copy()).float().div(255).mul(2).sub(1)


def _diffusion(golden, dim):
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    meta = golden("g11_img_scales.json")["C1"]
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    net.load_state_dict(closed_form_state_dict(dim))
    d = MultiScaleGaussianDiffusion(net, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"],
                                    image_sizes=[tuple(s) for s in meta["sizes"]], timesteps=meta["T"],
                                    train_full_t=True, scale_losses=meta["rescale_losses"], loss_factor=1,
                                    loss_type="l1", device=DEV, reblurring=True, omega=0).to(DEV)
    return net, d, meta


def test_l1_loss_kernel():
    from sinddm_amd.autograd import l1_loss
    a = hash_randn((3, 3, 37, 41), 1).to(DEV)
    b = hash_randn((3, 3, 37, 41), 2).to(DEV).requires_grad_(True)
    b.data[0, 0, 0, :5] = a[0, 0, 0, :5]          # exact ties -> sign(0) = 0
    loss = l1_loss(a, b)
    (loss * 0.5).backward()
    bc = b.detach().cpu().requires_grad_(True)
    ref = (a.cpu() - bc).abs().mean()
    (ref * 0.5).backward()
    assert abs(float(loss) - float(ref)) < 1e-6
    assert max_abs(b.grad.cpu(), bc.grad) < 1e-9


def test_adam_ema_kernels():
    from sinddm_amd.models import SinDDMNet
    from sinddm_amd.optim import FusedAdam, ema_update_
    net = SinDDMNet(dim=16, multiscale=True, device=DEV).to(DEV)
    ema = SinDDMNet(dim=16, multiscale=True, device=DEV).to(DEV)
    ema.load_state_dict(net.state_dict())
    opt = FusedAdam(net, lr=1e-3)
    p = net.flat_params.detach().cpu().clone()
    e = p.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for n in range(1, 6):
        g = hash_randn(tuple(p.shape), 100 + n) * (10.0 ** (n - 3))
        net.flat_grads.copy_(g.to(DEV))
        lr = O.multistep_lr(1e-3, [2, 4], n)
        opt.param_groups[0]["lr"] = lr
        opt.step()
        O.adam_step(p, g, m, v, n, lr)
        assert max_abs(net.flat_params.cpu(), p) < 2e-7, n
        ema_update_(ema, net, 0.995)
        e = O.ema_update(e, p, 0.995)
        assert max_abs(ema.flat_params.cpu(), e) < 2e-7, n
    # parameters seen through the nn.Parameter views are the updated ones
    assert max_abs(torch.cat([q.detach().reshape(-1) for q in net.parameters()]).cpu(), p) < 2e-7


@pytest.mark.parametrize("lt", ["l2", "l1_pred_img"])
def test_p_losses_other_loss_types_golden(golden, lt):
    """G17: loss_type 'l2' / 'l1_pred_img' (reference models.py:595-607; main.py hard-codes 'l1', VERDICT r4 missing 5):
    value and three gradient tensors against the reference, both branches of t[0] > 0."""
    g = golden("g17_loss_types.npz")
    pyr = golden("c1_pyramid.npz")
    net, d, meta = _diffusion(golden, 32)
    d.loss_type = lt
    net.bind_grads()
    for s in (0, 2):
        orig = _pyr_tensor(pyr[f"scale_{s}"])[None].repeat(2, 1, 1, 1).to(DEV)
        recon = _pyr_tensor(pyr[f"scale_{s}_recon"])[None].repeat(2, 1, 1, 1).to(DEV) if s > 0 else orig
        for tag, tt in (("a", [37, 5]), ("b", [0, 9])):
            net.flat_grads.zero_()
            t = torch.tensor(tt, device=DEV)
            noise = hash_randn(tuple(orig.shape), noise_key("train", s, 7)).to(DEV)
            loss = d.p_losses(recon, t, s, noise=noise, x_orig=orig) if s > 0 else d.p_losses(orig, t, s, noise=noise)
            loss.backward()
            key = f"{lt}_s{s}{tag}"
            ref = float(g[key + "_loss"])
            assert abs(float(loss) - ref) < 2e-6 * max(1.0, abs(ref)), key
            grads = {n: p.grad for n, p in net.named_parameters()}
            for pn in ("final_conv.0.weight", "l2.net.0.weight", "l1.ds_conv.weight"):
                assert rel_l2(grads[pn].cpu(), g[f"{key}_g_{pn}"]) < 1e-4, (key, pn)


def test_ema_copy_mode2_and_trainer_reset():
    """Mode 2 of sinddm_adam_ema_step (ema = p in one launch; VERDICT r4 item 6: declared in the ABI, never called):
    bit-exact copy of the flat buffer, the packed weights of the EMA network are rebuilt (its next evaluation uses the
    copied weights), and MultiscaleTrainer.reset_parameters / step_ema before step_start_ema go through it."""
    from sinddm_amd.models import SinDDMNet
    from sinddm_amd.optim import ema_copy_
    net = SinDDMNet(dim=16, multiscale=True, device=DEV).to(DEV)
    ema = SinDDMNet(dim=16, multiscale=True, device=DEV).to(DEV)
    net.load_state_dict(closed_form_state_dict(16))
    assert not torch.equal(net.flat_params, ema.flat_params)
    x = hash_randn((2, 3, 20, 24), 3).to(DEV)
    t = torch.tensor([5, 50], device=DEV)
    with torch.no_grad():
        y_before = ema(x, t, scale=1).clone()
        ema_copy_(ema, net)
        assert torch.equal(net.flat_params, ema.flat_params)
        y_net, y_ema = net(x, t, scale=1), ema(x, t, scale=1)
    assert torch.equal(y_net, y_ema) and not torch.equal(y_before, y_ema)


@pytest.mark.parametrize("s", [0, 2])
def test_p_losses_grads_golden(golden, s):
    """G5: loss value and all 52 parameter gradients of p_losses vs the reference (dim=32, B=2)."""
    g5 = golden("g5_losses.npz")
    pyr = golden("c1_pyramid.npz")
    net, d, meta = _diffusion(golden, 32)
    net.bind_grads()
    net.flat_grads.zero_()
    orig = _pyr_tensor(pyr[f"scale_{s}"])[None].repeat(2, 1, 1, 1).to(DEV)
    recon = _pyr_tensor(pyr[f"scale_{s}_recon"])[None].repeat(2, 1, 1, 1).to(DEV) if s > 0 else orig
    t = torch.tensor([37, 5], device=DEV)
    noise = hash_randn(tuple(orig.shape), noise_key("train", s, 0)).to(DEV)
    if s > 0:
        loss = d.p_losses(recon, t, s, noise=noise, x_orig=orig)
    else:
        loss = d.p_losses(orig, t, s, noise=noise)
    loss.backward()
    assert abs(float(loss) - float(g5[f"s{s}_loss"])) < 2e-6
    worst = 0.0
    for name, p in net.named_parameters():
        ref = g5[f"s{s}_g_{name}"]
        err = rel_l2(p.grad.cpu(), ref)
        worst = max(worst, err)
        assert err < 2e-4, (name, err)
    print("worst rel-l2 grad error", worst)


@pytest.mark.parametrize("dim,B,H,W", [(160, 2, 21, 37), (160, 1, 40, 70), (32, 3, 9, 33), (16, 1, 5, 7),
                                       (48, 2, 11, 35), (80, 2, 14, 40), (96, 1, 9, 33)])
def test_net_backward_vs_oracle_autograd(dim, B, H, W):
    """Parameter gradients AND input gradient vs torch autograd through the CPU oracle (ragged sizes)."""
    from sinddm_amd.models import SinDDMNet
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    net.load_state_dict(closed_form_state_dict(dim))
    net.bind_grads()
    net.flat_grads.zero_()
    x = hash_randn((B, 3, H, W), 5)
    gy = hash_randn((B, 3, H, W), 6)
    t = torch.arange(B) * 11 + 3
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd, t.to(DEV), scale=2)
    y.backward(gy.to(DEV))
    sd = {k: v.clone().requires_grad_(True) for k, v in closed_form_state_dict(dim).items()}
    xc = x.clone().requires_grad_(True)
    yc = O.net_forward(sd, xc, t, 2)
    yc.backward(gy)
    assert rel_l2(y.detach().cpu(), yc.detach()) < 1e-5
    assert rel_l2(xd.grad.cpu(), xc.grad) < 5e-5
    for name, p in net.named_parameters():
        err = rel_l2(p.grad.cpu(), sd[name].grad)
        assert err < 2e-4, (name, err)
    # gradients accumulate (+=) like autograd: a second backward doubles them
    y2 = net(x.to(DEV), t.to(DEV), scale=2)
    y2.backward(gy.to(DEV))
    for name, p in net.named_parameters():
        assert rel_l2(p.grad.cpu(), 2 * sd[name].grad) < 2e-4, name


def test_train_20_steps_golden(golden, tmp_path):
    """G10: 20 optimizer steps of MultiscaleTrainer.train() with injected (scale, t, noise): loss
    trajectory, LR schedule, final parameters and EMA parameters vs the reference run."""
    from sinddm_amd.trainer import MultiscaleTrainer
    g = golden("g10_train.npz")
    pyr = golden("c1_pyramid.npz")
    folder = str(tmp_path / "balloons") + "/"
    for key in pyr.files:
        os.makedirs(folder + key, exist_ok=True)
        Image.fromarray(pyr[key]).save(folder + key + "/balloons.png")
    net, d, meta = _diffusion(golden, 32)
    sizes = [tuple(s) for s in meta["sizes"]]
    tr = MultiscaleTrainer(d, folder=folder, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"],
                           image_sizes=sizes, train_batch_size=2, train_lr=1e-3, train_num_steps=20,
                           gradient_accumulate_every=1, ema_decay=0.995, fp16=False, step_start_ema=6,
                           update_ema_every=2, save_and_sample_every=10 ** 9, avg_window=100,
                           sched_milestones=[5, 12], results_folder=str(tmp_path / "res"), device=DEV)
    s_seq, t_seq = list(g["s_seq"]), g["t_seq"]
    tr.scale_fn = lambda step: s_seq[step]
    losses, lrs = [], []
    orig_forward = d.forward

    def rec_forward(x, s, *a, **k):
        loss = orig_forward(x, s, *a, **k)
        losses.append(loss.detach())
        lrs.append(tr.opt.param_groups[0]["lr"])
        return loss

    d.forward = rec_forward
    o_randint, o_randn_like = torch.randint, torch.randn_like
    torch.randint = lambda lo, hi, size, **kw: torch.tensor(t_seq[tr.step], dtype=torch.long, device=DEV)
    torch.randn_like = lambda x, **kw: hash_randn(tuple(x.shape), noise_key("train", s_seq[tr.step], tr.step)).to(x.device)
    try:
        tr.train()
    finally:
        torch.randint, torch.randn_like = o_randint, o_randn_like
    losses = np.array([float(l) for l in losses])
    assert np.allclose(np.array(lrs), g["lrs"], rtol=0, atol=1e-12)
    # the first step is identical to fp32 rounding; later steps drift slowly because Adam's update is
    # sign-like for small gradients (the same happens between two BLAS back-ends of the reference)
    assert abs(losses[0] - g["losses"][0]) < 2e-6
    assert (np.abs(losses - g["losses"]) / g["losses"]).max() < 2e-3, np.abs(losses - g["losses"]) / g["losses"]
    # Adam's m/sqrt(v) is sign-like for tiny gradients, so individual weights may differ by O(lr);
    # compare the parameter vectors as a whole
    pv = torch.cat([p.detach().reshape(-1) for p in tr.model.denoise_fn.parameters()]).cpu()
    ev = torch.cat([p.detach().reshape(-1) for p in tr.ema_model.denoise_fn.parameters()]).cpu()
    names = [n for n, _ in tr.model.denoise_fn.named_parameters()]
    rp = torch.cat([torch.from_numpy(g[f"p_{n}"]).reshape(-1) for n in names])
    re = torch.cat([torch.from_numpy(g[f"ema_{n}"]).reshape(-1) for n in names])
    p0 = torch.cat([v.reshape(-1) for v in closed_form_state_dict(32).values()])
    # relative to the distance actually travelled by the optimizer
    moved = float((rp - p0).norm())
    assert float((pv - rp).norm()) / moved < 2e-2, float((pv - rp).norm()) / moved
    assert float((ev - re).norm()) / float((re - p0).norm()) < 2e-2


def test_second_forward_before_backward_raises():
    """The training workspace holds ONE graph's activations; backward of an overwritten graph must fail loudly
    instead of returning wrong gradients."""
    from sinddm_amd import _lib
    from sinddm_amd.models import SinDDMNet
    net = SinDDMNet(dim=16, multiscale=True, device=DEV).to(DEV)
    x = hash_randn((1, 3, 12, 20), 3).to(DEV)
    t = torch.tensor([5], device=DEV)
    y1 = net(x, t, scale=0)
    y2 = net(x, t, scale=1)
    y2.sum().backward()
    with pytest.raises(_lib.SinddmError):
        y1.sum().backward()


def test_net_backward_full_size_vs_oracle_autograd():
    """The training shape of config C2: finest scale 186x248, dim = 160 (batch 2 bounds the oracle's CPU autograd;
    samples are independent in every kernel).  All 52 parameter gradients + the input gradient.

    The reference value is the oracle's autograd in FLOAT64; the tolerance of every tensor is calibrated by the error the
    oracle's own float32 autograd makes against it (3x the worst of the tensor's class, floor 5e-5): the sums over 46 128 pixels of white-noise
    gradients (condition path, depthwise bias) carry 3e-4..5e-4 of rounding noise in ANY fp32 evaluation, the CPU's
    included.  tools/bwd_bisect.py / profiles/r03_bwd_tolerance_bisect.txt: F(2x4), F(2x2) and direct-convolution data
    gradients sit at 5.7e-6 / 4.1e-6 / 4.0e-6 on the input gradient (CPU fp32: 3.8e-6) and 3.6e-4 / 3.1e-4 / 5.4e-4 on
    the condition path (CPU fp32: 4.3e-4) -- the widths are summation noise, not Winograd."""
    from sinddm_amd.models import SinDDMNet
    dim, B, H, W = 160, 2, 186, 248
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    net.load_state_dict(closed_form_state_dict(dim))
    net.bind_grads()
    net.flat_grads.zero_()
    x = hash_randn((B, 3, H, W), 15)
    gy = hash_randn((B, 3, H, W), 16) / (B * 3 * H * W)         # the scale an L1-mean loss hands to the net
    t = torch.tensor([731, 12])
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd, t.to(DEV), scale=4)
    y.backward(gy.to(DEV))

    def oracle(dtype):
        torch.set_default_dtype(dtype)
        try:
            sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in closed_form_state_dict(dim).items()}
            xc = x.to(dtype).clone().requires_grad_(True)
            yc = O.net_forward(sd, xc, t, 4)
            yc.backward(gy.to(dtype))
        finally:
            torch.set_default_dtype(torch.float32)
        return yc.detach(), xc.grad, {k: v.grad for k, v in sd.items()}

    y64, gx64, g64 = oracle(torch.float64)
    y32, gx32, g32 = oracle(torch.float32)
    assert rel_l2(y.detach().cpu().double(), y64) < 2e-6
    assert rel_l2(xd.grad.cpu().double(), gx64) < max(2e-5, 3 * rel_l2(gx32.double(), gx64))
    # per class of tensors (the condition path's and the biases' gradients are plain sums over all pixels, accumulated
    # with atomics on the GPU: their rounding noise varies from run to run): HIP error of every tensor < 3x the WORST
    # float32-CPU error in its class
    errs = {}
    for name, p in net.named_parameters():
        errs[name] = (rel_l2(p.grad.cpu().double(), g64[name]), rel_l2(g32[name].double(), g64[name]))
    cpu_worst = {}
    for name, (e, c) in errs.items():
        cpu_worst[klass(name)] = max(cpu_worst.get(klass(name), 0.0), c)
    for name, (e, c) in errs.items():
        assert e < max(5e-5, 3 * cpu_worst[klass(name)]), (name, e, c, cpu_worst)
        assert e < 1.5e-3, (name, e)
    worst = max(errs.items(), key=lambda kv: kv[1][0])
    print("full-size backward: worst rel-L2 gradient error vs float64 (HIP, CPU fp32)", worst, cpu_worst)


def test_net_backward_binary16_convs_vs_float64():
    """A training launch big enough for the binary16 hi/lo Winograd kernel (conv_wh.h: 8 x 186x248 = 12 items per CU):
    the forward 3x3 convs and both data-gradient convs of every block run on it (sinddm_debug_train_path = 8), fed by the
    per-sample running-max scalars of the training workspace (backward half: maintained by the depthwise data-gradient
    launches, the first conv's epilogue and one standalone pass over the final conv's data gradient).

    Gate, as for inference (tests/test_gpu_h2.py): against the FLOAT64 oracle autograd the binary16 path may not be worse than
    1.5x the fp32-MFMA path of the same library on the same inputs (per class of tensors, floor 5e-5: the condition path's
    sums over all pixels carry run-to-run atomics noise)."""
    from sinddm_amd import _lib
    from sinddm_amd.models import SinDDMNet
    lib = _lib.load()
    dim, B, H, W = 160, 8, 186, 248
    x = hash_randn((B, 3, H, W), 25)
    gy = hash_randn((B, 3, H, W), 26) / (B * 3 * H * W)
    t = torch.tensor([731, 12, 5, 999, 340, 77, 501, 888])

    def run(mode):
        try:
            assert lib.sinddm_debug_train_path(dim | (0 if mode == 3 else _lib.DIM_FP32_CONVS), B, H, W) == (8 if mode == 3 else 4)
            net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
            net.fp32_convs = mode != 3
            net.load_state_dict(closed_form_state_dict(dim))
            net.bind_grads()
            net.flat_grads.zero_()
            xd = x.to(DEV).requires_grad_(True)
            y = net(xd, t.to(DEV), scale=4)
            y.backward(gy.to(DEV))
            torch.cuda.synchronize()
            return (y.detach().cpu().double(), xd.grad.cpu().double(),
                    {n: p.grad.cpu().double().clone() for n, p in net.named_parameters()})
        finally:
            pass

    y_h, gx_h, g_h = run(3)
    y_f, gx_f, g_f = run(0)
    torch.set_default_dtype(torch.float64)
    try:
        sd = {k: v.double().clone().requires_grad_(True) for k, v in closed_form_state_dict(dim).items()}
        xc = x.double().clone().requires_grad_(True)
        yc = O.net_forward(sd, xc, t, 4)
        yc.backward(gy.double())
    finally:
        torch.set_default_dtype(torch.float32)
    y64, gx64, g64 = yc.detach(), xc.grad, {k: v.grad for k, v in sd.items()}
    e_y = (rel_l2(y_h, y64), rel_l2(y_f, y64))
    e_gx = (rel_l2(gx_h, gx64), rel_l2(gx_f, gx64))
    assert e_y[0] < 2e-6 and e_y[0] < 1.5 * e_y[1] + 1e-7, e_y
    assert e_gx[0] < 2e-5 and e_gx[0] < 1.5 * e_gx[1] + 1e-7, e_gx
    assert rel_l2(gx_h, gx_f) > 0                      # (the two paths are different kernels)

    errs = {n: (rel_l2(g_h[n], g64[n]), rel_l2(g_f[n], g64[n])) for n in g_h}
    worst_f = {}
    for n, (eh, ef) in errs.items():
        worst_f[klass(n)] = max(worst_f.get(klass(n), 0.0), ef)
    for n, (eh, ef) in errs.items():
        assert eh < max(5e-5, 1.5 * worst_f[klass(n)]), (n, eh, ef, worst_f)
    print("binary16 training convs vs float64: y", e_y, "grad_x", e_gx, "worst tensor",
          max(errs.items(), key=lambda kv: kv[1][0]), "fp32-path class worst", worst_f)


@pytest.mark.parametrize("B,H,W", [(1, 6, 192), (2, 13, 320), (1, 3, 516), (2, 9, 188)])
def test_depthwise_weight_gradient_kernels_vs_float64(B, H, W):
    """The depthwise 5x5 weight / bias / condition gradients of ONE block (sinddm_debug_block_train, block 1: 80 -> 160) on
    wide aligned images -- the register-window kernel (W % 4 == 0, W >= 192: one and several 256-column bands, fewer rows
    than waves) -- and on a width the LDS-tile kernel keeps (188), against a float64 torch evaluation of the block
    (reference SinDDM/models.py:69-80 under autograd)."""
    import torch.nn.functional as F
    from sinddm_amd import _lib
    from sinddm_amd.models import SinDDMNet, _workspace
    lib = _lib.load()
    dim, li, cin, cout = 160, 1, 80, 160
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    sd = closed_form_state_dict(dim)
    net.load_state_dict(sd)
    x = hash_randn((B, cin, H, W), 71)
    cb = 0.1 * hash_randn((B, cin), 72)
    gy = hash_randn((B, cout, H, W), 73) / (B * 3 * H * W)
    D = torch.float64
    xr = x.to(D).requires_grad_(True)
    cbr = cb.to(D).requires_grad_(True)
    w = {k: sd[f"l2.{k}"].to(D).requires_grad_(True) for k in ("ds_conv.weight", "ds_conv.bias", "net.0.weight", "net.0.bias",
                                                                "net.2.weight", "net.2.bias", "res_conv.weight", "res_conv.bias")}
    h = F.conv2d(xr, w["ds_conv.weight"], w["ds_conv.bias"], padding=2, groups=cin) + cbr[:, :, None, None]
    o = F.conv2d(F.gelu(F.conv2d(h, w["net.0.weight"], w["net.0.bias"], padding=1)), w["net.2.weight"], w["net.2.bias"], padding=1)
    o = o + F.conv2d(xr, w["res_conv.weight"], w["res_conv.bias"])
    o.backward(gy.to(D))
    ws = _workspace(DEV, lib.sinddm_train_workspace_bytes(dim, B, H, W), tag="train")
    y = torch.empty(B, cout, H, W, device=DEV)
    gx = torch.empty(B, cin, H, W, device=DEV)
    dc = torch.zeros(B, cin, device=DEV)
    gr = torch.zeros_like(net.flat_params)
    xd, cbd, gyd = x.to(DEV), cb.to(DEV), gy.to(DEV)
    _lib.check(lib.sinddm_debug_block_train(_lib.ptr(net.flat_params), _lib.ptr(net.packed_weights()), _lib.ptr(net.packed_weights_bwd()),
                                            dim, li, _lib.ptr(xd), _lib.ptr(cbd), _lib.ptr(gyd), _lib.ptr(y), _lib.ptr(gx), _lib.ptr(gr),
                                            _lib.ptr(dc), B, H, W, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV)), "sinddm_debug_block_train")
    torch.cuda.synchronize()
    assert rel_l2(y.cpu().double(), o.detach()) < 5e-6
    assert rel_l2(gx.cpu().double(), xr.grad) < 2e-5
    assert rel_l2(dc.cpu().double(), cbr.grad) < 5e-5
    gr = gr.cpu()
    for name, p in net.named_parameters():
        if name in ("l2.ds_conv.weight", "l2.ds_conv.bias"):
            off = (p.data_ptr() - net.flat_params.data_ptr()) // 4
            got = gr[off:off + p.numel()].reshape(p.shape).double()
            assert rel_l2(got, w[name[3:]].grad) < 5e-5, (name, rel_l2(got, w[name[3:]].grad))


def test_weight_gradients_reproducible_run_to_run():
    """Regression test of the LDS-DMA publication race: the same backward three times -- the only
    legitimate run-to-run difference is the order of the fp32 atomics (<= 1e-6 rel-L2); the race showed as 1e-4 .. 2e-3 in
    the 160-input-channel weight gradients (16-channel slab of wgrad_wino_wide_kernel)."""
    from sinddm_amd.models import SinDDMNet
    dim, B, H, W = 160, 24, 96, 128
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    net.load_state_dict(closed_form_state_dict(dim))
    net.bind_grads()
    x = hash_randn((B, 3, H, W), 5).to(DEV)
    gy = (hash_randn((B, 3, H, W), 6) / (B * 3 * H * W)).to(DEV)
    t = torch.tensor([(91 * (i + 1)) % 1000 for i in range(B)], dtype=torch.long, device=DEV)
    runs = []
    for _ in range(3):
        net.flat_grads.zero_()
        y = net(x.clone().requires_grad_(True), t, scale=3)
        y.backward(gy)
        runs.append(net.flat_grads.clone())
    for name, p in net.named_parameters():
        if p.dim() == 4 and p.shape[-1] == 3:
            a = p.grad
            off = a.data_ptr() - net.flat_grads.data_ptr()
            sl = slice(off // 4, off // 4 + a.numel())
            for r in (1, 2):
                assert rel_l2(runs[r][sl].cpu(), runs[0][sl].cpu()) < 2e-6, (name, r)
