"""Masked training on the GPU: per-pixel loss weights (MultiScaleGaussianDiffusion.train_weights), holes the weights never see.

p_losses takes sum(w e) / (B C sum w) in place of the mean; for 'l1' that is one fused kernel (sinddm_l1_loss_weighted_fwd_bwd:
the loss, the gradient, the zeros of the halo and of the holes).  tests/train_mask_util.py is the loss in float64 and the kernel
in numpy; tests/test_train_mask_host.py proves the receptive-radius statement in float64.  Here:

  1. the kernel against numpy: every element written, the halo and the w == 0 elements exactly 0, every other element bit-equal,
     the loss within 1e-6 of the float64 sum, a second call adding to the first;
  2. NaN / Inf wherever w == 0 and all over the halo change nothing;
  3. w = 1 is sinddm_l1_loss_crop_fwd_bwd (and, without a halo, sinddm_l1_loss_fwd_bwd), bit for bit in the gradient;
  4. p_losses + backward against the float64 restatement, plain and tiled, the three loss types;
  5. with the hole grown by 16 the step does not depend on what the hole holds; with grow = 0 it does;
  6. train_weights = None is the untouched step;
  7. MultiscaleTrainer(train_mask=...) builds the maps, fills the holes and trains.
dim 16, B = 2, the sizes of tests/test_gpu_tile_train.py; test 1's shapes: one float per thread and less than a block (5x7), one
halo axis each, both with W % 4 != 0, and 270 000 elements: past one pass of the kernel's grid."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from sinddm_amd import functions as F
from sinddm_amd.synth import hash_randn
from tile_train_util import halo_of
from train_mask_util import l1_weighted_reference, radius_case, weighted_p_losses_autograd
from train_step_util import DEV, inputs as _inputs, recorded_step, sched_and_diffusion as _sched_and_diffusion, step as _step

pytestmark = pytest.mark.gpu
NAME = "sinddm_l1_loss_weighted_fwd_bwd"

SHAPES = [(1, 5, 7, 0, 0), (2, 9, 13, 16, 0), (3, 8, 64, 0, 16), (2, 33, 130, 16, 16), (2, 150, 300, 0, 0)]


def _weight_map(kind, H, W, key):
    """'binary': a random {0,1} map; 'soft': values in [0, 1] with some exact zeros.  The pixels of _kernel_inputs' planted
    ties carry weight."""
    u = hash_randn((H, W), key)
    if kind == "binary":
        w = (u > 0).float()
    else:
        w = hash_randn((H, W), key + 1).abs().mul(0.5).clamp(0, 1)
        w[u < -0.4] = 0.0
    w[0, :3] = 1.0 if kind == "binary" else 0.75
    w[H - 1, W - 2:] = 1.0 if kind == "binary" else 0.375
    assert 0 < int((w == 0).sum()) < w.numel() and float(w.min()) >= 0.0
    return w.contiguous()


def _kernel_inputs(B, H, W, hy, hx):
    """(noise, eps_ext) on the CPU with five exact ties d == 0 planted in the centre."""
    noise = hash_randn((B, 3, H, W), 70 + W)
    eps_ext = hash_randn((B, 3, H + 2 * hy, W + 2 * hx), 71 + W)
    centre = eps_ext[:, :, hy:hy + H, hx:hx + W]
    centre[0, 0, 0, :3] = noise[0, 0, 0, :3]
    centre[-1, 2, H - 1, W - 2:] = noise[-1, 2, H - 1, W - 2:]
    return noise, eps_ext


def _inv_norm(B, w):
    return 1.0 / (B * 3 * float(w.to(torch.float64).sum()))


def _call(noise, eps_ext, w, halo, inv_norm, grad_scale, loss=None, guard=8):
    """One call of the entry on device copies, the gradient into a NaN-filled buffer with guard bands: (loss tensor, gradient
    (B,3,He,We) on the CPU).  The guards are checked here."""
    from sinddm_amd import _lib
    lib = _lib.load()
    B, _, H, W = noise.shape
    nz, ee, ww = noise.to(DEV).contiguous(), eps_ext.to(DEV).contiguous(), w.to(DEV).contiguous()
    big = torch.full((guard + ee.numel() + guard,), float("nan"), device=DEV)
    if loss is None:
        loss = torch.zeros((), device=DEV)
    _lib.check(getattr(lib, NAME)(_lib.ptr(nz), _lib.ptr(ee), _lib.ptr(ww), _lib.ptr(loss), big.data_ptr() + 4 * guard, B, 3, H,
                                  W, halo[0], halo[1], inv_norm, grad_scale, _lib.stream_ptr(DEV)), NAME)
    torch.cuda.synchronize()
    assert bool(big[:guard].isnan().all()) and bool(big[-guard:].isnan().all())
    return loss, big[guard:-guard].view(ee.shape).cpu()


# ---- 1: the kernel against numpy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["binary", "soft"])
@pytest.mark.parametrize("B,H,W,hy,hx", SHAPES, ids=lambda v: str(v))
def test_kernel_vs_numpy(B, H, W, hy, hx, kind):
    noise, eps_ext = _kernel_inputs(B, H, W, hy, hx)
    w = _weight_map(kind, H, W, 200 + W)
    inv = _inv_norm(B, w)
    l_ref, g_ref = l1_weighted_reference(noise, eps_ext, w, (hy, hx), inv, 0.5)
    loss, g = _call(noise, eps_ext, w, (hy, hx), inv, 0.5)
    g = g.numpy()
    assert not np.isnan(g).any()                                              # every element was written
    halo = g.copy()
    halo[:, :, hy:hy + H, hx:hx + W] = 0.0
    assert not halo.any()                                                     # exactly 0 on the halo
    off = np.broadcast_to(w.numpy() == 0, noise.shape)
    centre = g[:, :, hy:hy + H, hx:hx + W]
    assert not centre[off].any()                                              # and where w == 0
    assert np.array_equal(g, g_ref)                                           # every other element: bit-equal
    assert int((centre[~off] == 0).sum()) == 5                                # the planted ties, and only those
    err = abs(float(loss) - l_ref) / abs(l_ref)
    print(f"[{(B, H, W, hy, hx)} {kind}] loss {float(loss):.8g} vs {l_ref:.8g} ({err:.1e})")
    assert err <= 1e-6
    loss2, g2 = _call(noise, eps_ext, w, (hy, hx), inv, 0.5, loss=loss)       # a second call adds to loss_out
    assert loss2 is loss and np.array_equal(g2.numpy(), g_ref)
    assert abs(float(loss2) - 2 * l_ref) <= 1e-6 * abs(2 * l_ref)
    # the autograd wrapper: the same numbers, scaled by the upstream gradient
    from sinddm_amd.autograd import l1_loss
    e = eps_ext.to(DEV).requires_grad_(True)
    out = l1_loss(noise.to(DEV), e, (hy, hx), w.to(DEV), inv)
    (out * 0.5).backward()
    assert abs(float(out.detach()) - l_ref) <= 1e-6 * abs(l_ref)
    assert np.array_equal(e.grad.cpu().numpy(), g_ref)


# ---- 2: what a hole holds cannot reach the loss -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,hy,hx", [(1, 4, 6, 3, 2), (2, 9, 13, 16, 0), (2, 33, 130, 16, 16)], ids=lambda v: str(v))
def test_nan_and_inf_in_the_holes_and_the_halo(B, H, W, hy, hx):
    """NaN and +-Inf written into eps_ext wherever w == 0 and over the whole halo: the gradient is the clean run's (exactly 0
    there), the loss is finite and within 1e-6 of the float64 sum, which never saw those elements -- and bit-equal to the
    clean run's where the loss is one workgroup's sum (4x6 with its halo: 300 elements), which no atomic reorders."""
    noise, eps_ext = _kernel_inputs(B, H, W, hy, hx)
    w = _weight_map("soft", H, W, 300 + W)
    inv = _inv_norm(B, w)
    l_ref, g_ref = l1_weighted_reference(noise, eps_ext, w, (hy, hx), inv, 1.0)
    l_clean, g_clean = _call(noise, eps_ext, w, (hy, hx), inv, 1.0)
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.arange(eps_ext.numel()) % 3].view(eps_ext.shape)
    keep = torch.zeros(eps_ext.shape, dtype=torch.bool)
    keep[:, :, hy:hy + H, hx:hx + W] = (w > 0).expand(B, 3, H, W)
    poisoned = torch.where(keep, eps_ext, bad)
    assert int((~keep).sum()) > 0 and not bool(torch.isfinite(poisoned[~keep]).any())
    l_bad, g_bad = _call(noise, poisoned, w, (hy, hx), inv, 1.0)
    assert np.array_equal(g_clean.numpy(), g_ref) and np.array_equal(g_bad.numpy(), g_ref)
    assert not g_bad[~keep].any()
    assert np.isfinite(float(l_bad))
    for l in (l_clean, l_bad):
        assert abs(float(l) - l_ref) <= 1e-6 * abs(l_ref)
    if eps_ext.numel() <= 512:
        assert float(l_bad) == float(l_clean)


# ---- 3: w = 1 is the crop kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,hy,hx", SHAPES[:4], ids=lambda v: str(v))
def test_unit_weights_are_the_crop_kernel(B, H, W, hy, hx):
    from sinddm_amd import _lib
    lib = _lib.load()
    noise, eps_ext = _kernel_inputs(B, H, W, hy, hx)
    n = B * 3 * H * W
    inv = float(np.float32(1) / np.float32(n))
    loss, g = _call(noise, eps_ext, torch.ones(H, W), (hy, hx), inv, 0.5)
    nz, ee = noise.to(DEV), eps_ext.to(DEV)
    st = _lib.stream_ptr(DEV)
    l_crop, g_crop = torch.zeros((), device=DEV), torch.full_like(ee, float("nan"))
    _lib.check(lib.sinddm_l1_loss_crop_fwd_bwd(_lib.ptr(nz), _lib.ptr(ee), _lib.ptr(l_crop), _lib.ptr(g_crop), B * 3, H, W, hy, hx,
                                               0.5, st), "sinddm_l1_loss_crop_fwd_bwd")
    torch.cuda.synchronize()
    assert torch.equal(g, g_crop.cpu())
    assert abs(float(loss) - float(l_crop)) <= 1e-6 * abs(float(l_crop))
    if (hy, hx) == (0, 0):
        l_plain, g_plain = torch.zeros((), device=DEV), torch.full_like(ee, float("nan"))
        _lib.check(lib.sinddm_l1_loss_fwd_bwd(_lib.ptr(nz), _lib.ptr(ee), _lib.ptr(l_plain), _lib.ptr(g_plain), n, 0.5, st),
                   "sinddm_l1_loss_fwd_bwd")
        torch.cuda.synchronize()
        assert torch.equal(g, g_plain.cpu())


# ---- 4: p_losses against the float64 restatement --------------------------------------------------------------------------------------
P_CASES = [(0, "off", "l1", 9, 12), (1, "off", "l1", 12, 20), (0, "xy", "l1", 9, 12), (1, "xy", "l1", 12, 20),
           (1, "off", "l2", 9, 12), (1, "xy", "l1_pred_img", 9, 12)]


@pytest.mark.parametrize("s,tile,lt,H,W", P_CASES, ids=lambda v: str(v))
def test_p_losses_vs_float64(golden, s, tile, lt, H, W):
    """Loss < 1e-5 relative and all 52 parameter gradients < 2e-4 rel-L2 against weighted_p_losses_autograd in float64 (the
    bounds tests/test_gpu_train.py::test_net_backward_vs_oracle_autograd and tests/test_gpu_tile_train.py hold these kernels
    to); the UNWEIGHTED float64 gradient lies more than 1e-2 away in the worst tensor, so the comparison can tell."""
    net, d, sd, sched = _sched_and_diffusion(golden, 16, loss_type=lt)
    wrap = (True, True) if tile == "xy" else (False, False)
    x_start, x_orig, noise, t = _inputs(2, H, W, 700 + 10 * s + H)
    w = _weight_map("soft", H, W, 710 + s)
    d.train_tile = wrap
    d.train_weights = [w.to(DEV)] * d.n_scales
    loss, grads = _step(net, d, x_start, x_orig, noise, t, s)
    xo = x_orig if s > 0 else None
    l_ref, g_ref = weighted_p_losses_autograd(sched, sd, x_start, xo, t, s, noise, w, wrap, lt)
    _, g_flat = weighted_p_losses_autograd(sched, sd, x_start, xo, t, s, noise, torch.ones(H, W), wrap, lt)
    errs = {k: rel_l2(grads[k], g_ref[k]) for k in g_ref}
    apart = max(rel_l2(g_flat[k], g_ref[k]) for k in g_ref)
    print(f"[s={s} {tile} {lt} {H}x{W}] loss {loss:.7g} vs {l_ref:.7g} ({abs(loss - l_ref) / abs(l_ref):.1e}); worst gradient "
          f"{max(errs.values()):.2e} ({max(errs, key=errs.get)}); unweighted vs weighted {apart:.3f}")
    assert len(errs) == 52
    assert abs(loss - l_ref) < 1e-5 * abs(l_ref)
    for k, e in errs.items():
        assert e < 2e-4, (k, e)
    assert apart > 1e-2


# ---- 5: the weights never see the hole ------------------------------------------------------------------------------------------------
def test_step_does_not_depend_on_what_the_hole_holds(golden):
    """The set-up of tests/test_train_mask_host.py's float64 statement through p_losses at scale 1 (x_orig takes part), the
    same t and noise: the hole of x_start, x_orig and noise holds +0.9 in one run, -0.9 in the other.  grow = 16: the loss and
    every parameter gradient agree within 4e-4 rel-L2, tests/test_gpu_tile_train.py's bound for two device gradients that
    are equal in exact arithmetic (the Winograd tiles that straddle the hole's surroundings round differently).  grow = 0:
    the worst tensor differs by more than 1e-2."""
    _, _, t, valid, runs = radius_case(golden)
    net, d, _, _ = _sched_and_diffusion(golden, 16)
    for grow in (16, 0):
        (w,) = F.train_weight_pyramid(valid, [(48, 64)], grow=grow)
        d.train_weights = [None, w.to(DEV)]
        (la, ga), (lb, gb) = (_step(net, d, xs, xo, nz, t, 1) for xs, xo, nz in runs)
        diff = {k: rel_l2(ga[k], gb[k]) for k in gb}
        print(f"[grow {grow}] loss {abs(la - lb) / abs(lb):.1e}; gradients {min(diff.values()):.1e} .. {max(diff.values()):.1e}")
        if grow == 16:
            assert abs(la - lb) < 4e-4 * abs(lb)
            for k, e in diff.items():
                assert e < 4e-4, (k, e)
        else:
            assert max(diff.values()) > 1e-2


# ---- 6: nothing changes when off -------------------------------------------------------------------------------------------------------
def _recorded_step(golden, touch, x_start, x_orig, noise, t, s, monkeypatch):
    """One plain step on a fresh diffusion object (train_step_util.recorded_step), during which the weighted kernel's entry
    refuses to run.  `touch`: the object first ran a WEIGHTED step, then had train_weights set back to None."""
    net, d, _, _ = _sched_and_diffusion(golden, 16)
    if touch:
        d.train_weights = [_weight_map("soft", 7, 12, 800).to(DEV)] * d.n_scales
        weighted, _ = _step(net, d, x_start, x_orig, noise, t, s)
        d.train_weights = None
    rec = recorded_step(monkeypatch, net, d, x_start, x_orig, noise, t, s, (NAME,),
                        "the weighted kernel ran with train_weights = None")
    if touch:
        assert weighted != rec["loss"]                                         # (the weighted step was another step)
    return rec


@pytest.mark.parametrize("s", [0, 2])
def test_off_is_the_untouched_step(golden, monkeypatch, s):
    """train_weights = None, set explicitly after a weighted step, against a diffusion object whose attribute was never
    touched (dim 16, B = 2, 7x12: the loss is the sum of two workgroups' partial sums, which commutes).  The rule of
    tests/test_gpu_tile_train.py::test_off_is_the_untouched_step: sinddm_l1_loss_weighted_fwd_bwd is not called; the loss, x_noisy, the
    network's output and the gradient handed to its backward are bit-equal; the flat gradient buffer, which the backward
    kernels accumulate with fp32 atomics in an order that varies run to run, is held to 2e-6 rel-L2 per tensor -- as is the
    untouched object run twice."""
    x_start, x_orig, noise, t = _inputs(2, 7, 12, 600)
    a = _recorded_step(golden, False, x_start, x_orig, noise, t, s, monkeypatch)
    a2 = _recorded_step(golden, False, x_start, x_orig, noise, t, s, monkeypatch)
    b = _recorded_step(golden, True, x_start, x_orig, noise, t, s, monkeypatch)
    for other, what in ((a2, "untouched, again"), (b, "train_weights = None")):
        assert other["loss"] == a["loss"], what
        for k in ("x_noisy", "eps", "grad_eps"):
            assert torch.equal(other[k], a[k]), (what, k)
        for n, off in a["named"].items():
            sl = slice(off, off + a["numel"][n])
            assert rel_l2(other["flat_grads"][sl], a["flat_grads"][sl]) < 2e-6, (what, n)
    assert float(a["flat_grads"].abs().sum()) > 0


# ---- 7: the trainer ---------------------------------------------------------------------------------------------------------------
def test_trainer_trains_under_a_mask(golden, tmp_path):
    """MultiscaleTrainer(train_mask=..., train_mask_grow=[...]) over the C1 pyramid of tests/golden/balloons.png: one map per
    scale of that scale's size, the hole pixels of data_list filled, and two optimizer steps (the coarsest and the finest
    scale, through scale_fn) give finite losses and move the parameters."""
    from PIL import Image
    from sinddm_amd.trainer import MultiscaleTrainer
    pyr = golden("c1_pyramid.npz")
    folder = str(tmp_path / "balloons") + "/"
    for key in pyr.files:
        os.makedirs(folder + key, exist_ok=True)
        Image.fromarray(pyr[key]).save(folder + key + "/balloons.png")
    meta = golden("g11_img_scales.json")["C1"]
    net, d, _, _ = _sched_and_diffusion(golden, 16)
    n = meta["n_scales"]
    hw = [tuple(d.image_sizes[s]) for s in range(n)]
    valid = torch.ones(hw[-1])
    valid[30:50, 20:40] = 0
    grow = [0] * (n - 1) + [16]
    tr = MultiscaleTrainer(d, folder=folder, n_scales=n, scale_factor=meta["scale_factor"],
                           image_sizes=[tuple(v) for v in meta["sizes"]], train_batch_size=2, train_lr=1e-3, train_num_steps=2,
                           gradient_accumulate_every=1, save_and_sample_every=10 ** 9, results_folder=str(tmp_path / "res"),
                           device=DEV, train_mask=valid, train_mask_grow=grow)
    want = F.train_weight_pyramid(valid, hw, grow=grow)
    hard = F.keep_mask_pyramid(valid, hw, hard=True)
    assert tr.ema_model.train_weights is None and len(tr.model.train_weights) == n
    for s in range(n):
        w = tr.model.train_weights[s]
        assert w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == hw[s] and torch.equal(w.cpu(), want[s])
        hole = hard[s] < 0.5
        for img in tr.data_list[s]:
            img = img.cpu()
            for c in range(3):
                mean = img[0, c][~hole].to(torch.float64).mean().to(torch.float32)
                assert torch.equal(img[0, c][hole], mean.expand(int(hole.sum())))
    seq = [0, n - 1]
    tr.scale_fn = lambda step: seq[step]
    losses, before = [], net.flat_params.detach().clone()
    forward = d.forward
    d.forward = lambda x, s, *a, **k: losses.append(forward(x, s, *a, **k)) or losses[-1]
    tr.train()
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(bool(torch.isfinite(l)) and float(l) > 0 for l in losses)
    assert bool(torch.isfinite(net.flat_params).all()) and not torch.equal(net.flat_params, before)
