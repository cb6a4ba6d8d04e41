"""Crop training on the GPU: random windows per sample (MultiScaleGaussianDiffusion.train_crop), the loss on what the network saw
whole.

p_losses reads x_start / x_orig through one window per sample (sinddm_q_sample_crop), runs the network on the windows and takes
the loss on each window's valid rectangle (sinddm_l1_loss_rect_fwd_bwd).  tests/crop_train_util.py is the step in float64 and the
loss kernel in numpy; tests/test_crop_train_host.py proves the receptive-radius statement in float64.  Here:

  1. sinddm_q_sample_crop against sinddm_q_sample on a full-size noise whose windows hold the crop's noise: bit-equal;
  2. sinddm_l1_loss_rect_fwd_bwd against numpy: every element written, exactly 0 outside the rectangles and where w == 0, every
     other element bit-equal, the loss within 1e-6 of the float64 sum, a second call adding to the first;
  3. NaN / Inf outside the rectangles and where w == 0 change nothing;
  4. full rectangles without a map are sinddm_l1_loss_fwd_bwd, bit for bit in the gradient;
  5. p_losses + backward against the float64 restatement, the three loss types, with and without a map;
  6. the statement on the device: the cropped step against the two full-image masked steps;
  7. train_crop = None is the untouched step;  8. so is a scale not larger than the crop;
  9. MultiscaleTrainer(train_crop=...) trains, and raises when no window holds weight.
dim 16, B = 2 unless the shape list says otherwise."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from crop_train_util import (combine_by_area, crop_p_losses_autograd, l1_rect_reference, place_windows, rect_of, statement_case,
                             window_mask)
from sinddm_amd.synth import hash_randn
from train_step_util import (DEV, count_entries, inputs as _inputs, recorded_step, sched_and_diffusion as _sched_and_diffusion,
                             step as _step)

pytestmark = pytest.mark.gpu
Q_NAME, L_NAME = "sinddm_q_sample_crop", "sinddm_l1_loss_rect_fwd_bwd"

# (B, H, W, h, w): less than a block; one axis whole; w % 4 == 0 with odd x0; w % 4 != 0; 243 600 elements
SHAPES = [(1, 5, 7, 3, 4), (2, 9, 13, 9, 6), (3, 33, 130, 17, 64), (2, 33, 130, 16, 61), (2, 150, 300, 140, 290)]
ORIGINS = {(1, 5, 7, 3, 4): [[(0, 0)], [(0, 3)], [(2, 0)], [(2, 3)]],                     # the four corners in turn
           (2, 9, 13, 9, 6): [[(0, 1), (0, 7)]],
           (3, 33, 130, 17, 64): [[(0, 1), (16, 65), (7, 33)]],
           (2, 33, 130, 16, 61): [[(3, 0), (17, 69)]],
           (2, 150, 300, 140, 290): [[(10, 10), (0, 3)]],
           # past one pass of sinddm_q_sample_crop's grid (4096 blocks of 256): 16-byte accesses, and one float per thread
           (1, 610, 612, 600, 600): [[(9, 11)]], (1, 610, 612, 600, 601): [[(10, 5)]]}


def _lib_and_tables(golden):
    from sinddm_amd import _lib
    _, d, _, _ = _sched_and_diffusion(golden, 16)
    return _lib, _lib.load(), d


def _int32(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV).contiguous()


# ---- 1: sinddm_q_sample_crop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,h,w", SHAPES + [(1, 610, 612, 600, 600), (1, 610, 612, 600, 601)], ids=lambda v: str(v))
def test_q_sample_crop_is_q_sample_sliced(golden, B, H, W, h, w):
    """Scale 0 (no x_orig) and scale 2 (the gamma mix), a t per sample and a host t; the output goes into a NaN-filled buffer
    with guard bands -- and, once per shape, into one that is NOT 16-byte aligned (the rounding must not follow the output's
    alignment: it is that of sinddm_q_sample on the full-size tensors)."""
    _lib, lib, d = _lib_and_tables(golden)
    x0, xo, _, t = (v.to(DEV) for v in _inputs(B, H, W, 40 + W))
    nz = hash_randn((B, 3, h, w), 45 + w).to(DEV)
    nz_full = hash_randn((B, 3, H, W), 46 + W).to(DEV)
    gamma_row = d.gammas[1].reshape(-1).contiguous()
    assert 0.0 < float(gamma_row[7]) < 1.0
    for windows in ORIGINS[(B, H, W, h, w)]:
        full_noise = place_windows(nz_full, nz, windows)
        win = _int32(windows)
        for with_orig in (False, True):
            for t_dev, t_host, guard in ((t, 0, 8), (None, 31, 8), (t, 0, 7)):
                if guard == 7 and not with_orig:
                    continue
                full = d._q_sample_impl(x0, t_dev, t_host, full_noise, x_orig=xo if with_orig else None,
                                        gamma_row=gamma_row if with_orig else None)
                want = torch.stack([full[b, :, y0:y0 + h, x0_:x0_ + w] for b, (y0, x0_) in enumerate(windows)])
                big = torch.full((guard + nz.numel() + guard,), float("nan"), device=DEV)
                rc = lib.sinddm_q_sample_crop(_lib.ptr(x0), _lib.ptr(xo) if with_orig else None, _lib.ptr(nz),
                                              big.data_ptr() + 4 * guard, _lib.ptr(d.sqrt_alphas_cumprod),
                                              _lib.ptr(d.sqrt_one_minus_alphas_cumprod),
                                              _lib.ptr(gamma_row) if with_orig else None,
                                              _lib.ptr(t_dev) if t_dev is not None else None, t_host, _lib.ptr(win), B, 3, H, W, h, w,
                                              _lib.stream_ptr(DEV))
                torch.cuda.synchronize()
                assert rc == 0
                got = big[guard:-guard].view(B, 3, h, w)
                assert torch.equal(got, want), (windows, with_orig, t_host, guard)
                assert bool(big[:guard].isnan().all()) and bool(big[-guard:].isnan().all())
        # the Python route of p_losses is this call
        assert torch.equal(d._q_sample_impl(x0, t, 0, nz, x_orig=xo, gamma_row=gamma_row, crop=(h, w), windows=win), want)


@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (2, 12, 20)], ids=lambda v: str(v))
def test_q_sample_crop_of_the_whole_image_is_q_sample(golden, B, H, W):
    _lib, lib, d = _lib_and_tables(golden)
    x0, xo, nz, t = (v.to(DEV) for v in _inputs(B, H, W, 50 + W))
    gamma_row = d.gammas[1].reshape(-1).contiguous()
    win = _int32([(0, 0)] * B)
    for with_orig in (False, True):
        kw = dict(x_orig=xo, gamma_row=gamma_row) if with_orig else {}
        assert torch.equal(d._q_sample_impl(x0, t, 0, nz, crop=(H, W), windows=win, **kw), d._q_sample_impl(x0, t, 0, nz, **kw))


# ---- 2: sinddm_l1_loss_rect_fwd_bwd against numpy ------------------------------------------------------------------------------
L_SHAPES = SHAPES + [(2, 160, 320, 156, 300)]                                # 280 800 elements: past one pass of the kernel's grid


def _soft_map(H, W, key):
    """Values in [0, 1] with some exact zeros."""
    u = hash_randn((H, W), key)
    m = hash_randn((H, W), key + 1).abs().mul(0.5).clamp(0, 1)
    m[u < -0.4] = 0.0
    assert 0 < int((m == 0).sum()) < m.numel()
    return m.contiguous()


def _rects_for(B, h, w):
    """One rectangle per sample, by the shape: over the shape list a full window, an inner rectangle, one pixel and an empty
    rectangle all occur, the full and the empty one in one batch too."""
    kinds = dict(full=(0, h, 0, w), inner=(h // 3, h - h // 4, w // 4, w - w // 3), pixel=(h // 2, h // 2 + 1, w // 2, w // 2 + 1),
                 empty=(2, 2, 0, w), wide=(0, h, 1, w))
    pick = {(1, 3): ["wide"], (2, 9): ["full", "pixel"], (3, 17): ["inner", "empty", "full"], (2, 16): ["pixel", "inner"],
            (2, 140): ["full", "empty"], (2, 156): ["inner", "full"]}[(B, h)]
    return [kinds[k] for k in pick]


def _loss_inputs(B, H, W, h, w, rects, wmap, windows):
    """(noise, eps) window-size on the CPU with up to three exact ties d == 0 planted in the top row of the first rectangles
    that are at least two pixels wide, at pixels that carry weight (one pixel of the row is always left): returns the count
    planted too."""
    noise = hash_randn((B, 3, h, w), 70 + w)
    eps = hash_randn((B, 3, h, w), 71 + w)
    planted = 0
    for b, (ylo, yhi, xlo, xhi) in enumerate(rects):
        for x in range(xlo, xhi - 1):
            if yhi > ylo and planted < 3 and (wmap is None or float(wmap[windows[b][0] + ylo, windows[b][1] + x]) > 0):
                eps[b, 1, ylo, x] = noise[b, 1, ylo, x]
                planted += 1
    assert planted > 0
    return noise, eps, planted


def _call_loss(noise, eps, wmap, windows, rects, inv_norm, grad_scale, loss=None, guard=8):
    """One call of the entry on device copies, the gradient into a NaN-filled buffer with guard bands: (loss tensor, gradient
    on the CPU).  The guards are checked here."""
    from sinddm_amd import _lib
    lib = _lib.load()
    B, _, h, w = noise.shape
    nz, ee = noise.to(DEV).contiguous(), eps.to(DEV).contiguous()
    ww = wmap.to(DEV).contiguous() if wmap is not None else None
    win, rc = _int32(windows), _int32(rects)
    big = torch.full((guard + ee.numel() + guard,), float("nan"), device=DEV)
    if loss is None:
        loss = torch.zeros((), device=DEV)
    Hm, Wm = (wmap.shape if wmap is not None else (0, 0))
    _lib.check(getattr(lib, L_NAME)(_lib.ptr(nz), _lib.ptr(ee), _lib.ptr(ww), _lib.ptr(win), _lib.ptr(rc), _lib.ptr(loss),
                                    big.data_ptr() + 4 * guard, B, 3, h, w, Hm, Wm, inv_norm, grad_scale, _lib.stream_ptr(DEV)),
               L_NAME)
    torch.cuda.synchronize()
    assert bool(big[:guard].isnan().all()) and bool(big[-guard:].isnan().all())
    return loss, big[guard:-guard].view(ee.shape).cpu()


def _norm(rects, windows, wmap):
    from crop_train_util import brute_norm
    return 1.0 / (3 * brute_norm(windows, rects, None if wmap is None else wmap.numpy()))


@pytest.mark.parametrize("mapped", [False, True], ids=["no-map", "soft-map"])
@pytest.mark.parametrize("B,H,W,h,w", L_SHAPES, ids=lambda v: str(v))
def test_loss_kernel_vs_numpy(B, H, W, h, w, mapped):
    windows = ORIGINS[(B, H, W, h, w)][-1] if (B, H, W, h, w) in ORIGINS else [(2, 7), (4, 20)]
    rects = _rects_for(B, h, w)
    wmap = _soft_map(H, W, 200 + W) if mapped else None
    noise, eps, planted = _loss_inputs(B, H, W, h, w, rects, wmap, windows)
    inv = _norm(rects, windows, wmap)
    l_ref, g_ref, on = l1_rect_reference(noise, eps, wmap, windows, rects, inv, 0.5)
    loss, g = _call_loss(noise, eps, wmap, windows, rects, inv, 0.5)
    g = g.numpy()
    assert not np.isnan(g).any()                                              # every element was written
    assert not g[~on].any()                                                   # exactly 0 outside the rectangles and where w == 0
    assert np.array_equal(g, g_ref)                                           # every other element: bit-equal
    assert int((g[on] == 0).sum()) == planted                                 # the planted ties, and only those
    err = abs(float(loss) - l_ref) / abs(l_ref)
    print(f"[{(B, H, W, h, w)} {'map' if mapped else 'flat'}] loss {float(loss):.8g} vs {l_ref:.8g} ({err:.1e})")
    assert err <= 1e-6
    loss2, g2 = _call_loss(noise, eps, wmap, windows, rects, inv, 0.5, loss=loss)         # a second call adds to loss_out
    assert loss2 is loss and np.array_equal(g2.numpy(), g_ref)
    assert abs(float(loss2) - 2 * l_ref) <= 1e-6 * abs(2 * l_ref)
    # the autograd wrapper: the same numbers, scaled by the upstream gradient
    from sinddm_amd.autograd import l1_loss
    e = eps.to(DEV).requires_grad_(True)
    out = l1_loss(noise.to(DEV), e, (0, 0), wmap.to(DEV) if mapped else None, inv, _int32(windows), _int32(rects))
    (out * 0.5).backward()
    assert abs(float(out.detach()) - l_ref) <= 1e-6 * abs(l_ref)
    assert np.array_equal(e.grad.cpu().numpy(), g_ref)


# ---- 3: what lies outside a rectangle or under w == 0 cannot reach the loss -----------------------------------------------------
@pytest.mark.parametrize("B,H,W,h,w", [(1, 5, 7, 3, 4), (2, 9, 13, 9, 6), (2, 33, 130, 16, 61)], ids=lambda v: str(v))
def test_nan_and_inf_outside_the_rectangles_and_in_the_holes(B, H, W, h, w):
    """NaN and +-Inf written into eps AND noise wherever the element is outside its rectangle or has w == 0: the gradient is the
    clean run's, the loss is finite and within 1e-6 of the float64 sum -- and bit-equal to the clean run's where the loss is
    one workgroup's sum (36 elements), which no atomic reorders."""
    windows = ORIGINS[(B, H, W, h, w)][-1]
    rects = _rects_for(B, h, w)
    wmap = _soft_map(H, W, 300 + W)
    noise, eps, _ = _loss_inputs(B, H, W, h, w, rects, wmap, windows)
    inv = _norm(rects, windows, wmap)
    l_ref, g_ref, on = l1_rect_reference(noise, eps, wmap, windows, rects, inv, 1.0)
    l_clean, g_clean = _call_loss(noise, eps, wmap, windows, rects, inv, 1.0)
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.arange(eps.numel()) % 3].view(eps.shape)
    keep = torch.from_numpy(on.copy())
    assert int((~keep).sum()) > 0
    l_bad, g_bad = _call_loss(torch.where(keep, noise, bad.flip(0)), torch.where(keep, eps, bad), wmap, windows, rects, inv, 1.0)
    assert np.array_equal(g_clean.numpy(), g_ref) and np.array_equal(g_bad.numpy(), g_ref)
    assert not g_bad[~keep].any()
    assert np.isfinite(float(l_bad))
    for l in (l_clean, l_bad):
        assert abs(float(l) - l_ref) <= 1e-6 * abs(l_ref)
    if eps.numel() <= 512:
        assert float(l_bad) == float(l_clean)


# ---- 4: full rectangles without a map are the plain kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,h,w", SHAPES[:4], ids=lambda v: str(v))
def test_full_rectangles_are_the_plain_kernel(B, H, W, h, w):
    from sinddm_amd import _lib
    lib = _lib.load()
    rects = [(0, h, 0, w)] * B
    noise, eps, _ = _loss_inputs(B, H, W, h, w, rects, None, [(0, 0)] * B)
    n = B * 3 * h * w
    inv = float(np.float32(1) / np.float32(n))
    loss, g = _call_loss(noise, eps, None, [(0, 0)] * B, rects, inv, 0.5)
    nz, ee = noise.to(DEV), eps.to(DEV)
    l_plain, g_plain = torch.zeros((), device=DEV), torch.full_like(ee, float("nan"))
    _lib.check(lib.sinddm_l1_loss_fwd_bwd(_lib.ptr(nz), _lib.ptr(ee), _lib.ptr(l_plain), _lib.ptr(g_plain), n, 0.5,
                                          _lib.stream_ptr(DEV)), "sinddm_l1_loss_fwd_bwd")
    torch.cuda.synchronize()
    assert torch.equal(g, g_plain.cpu())
    assert abs(float(loss) - float(l_plain)) <= 1e-6 * abs(float(l_plain))


# ---- 5: p_losses against the float64 restatement ----------------------------------------------------------------------------------
def _crop_step(net, d, x_start, x_orig, noise, t, s, windows):
    """p_losses + backward with explicit windows: (loss as a float, {name: grad on the CPU})."""
    net.bind_grads()
    net.flat_grads.zero_()
    kw = dict(x_orig=x_orig.to(DEV)) if s > 0 else {}
    loss = d.p_losses(x_start.to(DEV), t.to(DEV), s, noise=noise.to(DEV), windows=torch.tensor(windows), **kw)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()}


# (s, loss type, window, margin, windows, a map?)   full size 12x20
P_CASES = [(0, "l1", (9, 12), 2, [(0, 3), (3, 8)], False), (1, "l1", (9, 12), 2, [(0, 3), (3, 8)], False),
           (1, "l1", (12, 12), 0, [(0, 2), (0, 8)], False), (1, "l2", (9, 12), 2, [(1, 0), (3, 5)], False),
           (1, "l1_pred_img", (9, 12), 2, [(0, 3), (3, 8)], False), (1, "l1", (9, 12), 2, [(2, 3), (3, 8)], True)]


@pytest.mark.parametrize("s,lt,window,m,windows,mapped", P_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_p_losses_vs_float64(golden, s, lt, window, m, windows, mapped):
    """Loss < 1e-5 relative and all 52 parameter gradients < 2e-4 rel-L2 against crop_p_losses_autograd in float64 (the bounds
    of tests/test_gpu_train_mask.py).  So that the comparison can tell, the float64 gradient of ANOTHER loss lies more than
    1e-2 away in the worst tensor: the whole-window loss (margin 0) -- or, in the case whose margin is 0 already, the same
    windows one column further left."""
    H, W = 12, 20
    net, d, sd, sched = _sched_and_diffusion(golden, 16, loss_type=lt)
    x_start, x_orig, _, t = _inputs(2, H, W, 700 + 10 * s + H)
    noise = hash_randn((2, 3, *window), 705 + s)
    wmap = _soft_map(H, W, 710 + s) if mapped else None
    d.train_crop, d.train_crop_margin = window, m
    if mapped:
        d.train_weights = [wmap.to(DEV)] * d.n_scales
    loss, grads = _crop_step(net, d, x_start, x_orig, noise, t, s, windows)
    xo = x_orig if s > 0 else None
    rects = [rect_of(o, (H, W), window, m) for o in windows]
    mask = window_mask(2, window, rects, windows, wmap)
    l_ref, g_ref = crop_p_losses_autograd(sched, sd, x_start, xo, t, s, noise, mask, windows, lt)
    if m > 0:
        other = window_mask(2, window, [rect_of(o, (H, W), window, 0) for o in windows], windows, wmap)
        _, g_other = crop_p_losses_autograd(sched, sd, x_start, xo, t, s, noise, other, windows, lt)
    else:
        shifted = [(y, x - 1) for y, x in windows]
        _, g_other = crop_p_losses_autograd(sched, sd, x_start, xo, t, s, noise, mask, shifted, lt)
    errs = {k: rel_l2(grads[k], g_ref[k]) for k in g_ref}
    apart = max(rel_l2(g_other[k], g_ref[k]) for k in g_ref)
    print(f"[s={s} {lt} {window} m={m}{' map' if mapped else ''}] loss {loss:.7g} vs {l_ref:.7g} "
          f"({abs(loss - l_ref) / abs(l_ref):.1e}); worst gradient {max(errs.values()):.2e} ({max(errs, key=errs.get)}); "
          f"the other loss {apart:.3f}")
    assert len(errs) == 52
    assert abs(loss - l_ref) < 1e-5 * abs(l_ref)
    for k, e in errs.items():
        assert e < 2e-4, (k, e)
    assert apart > 1e-2


# ---- 6: the statement on the device ---------------------------------------------------------------------------------------------------
def test_crop_step_is_a_masked_full_image_step(golden):
    """The set-up of tests/test_crop_train_host.py's float64 statement: the cropped step at B = 2 against the two B = 1
    full-image masked steps (train_weights = 1_{V_b}), combined by area.  margin 16: the loss and every parameter gradient
    agree within 4e-4 rel-L2, the project's bound for two device gradients that are equal in exact arithmetic.  margin 0:
    the worst tensor differs by more than 1e-2."""
    case = statement_case(golden)
    net, d, _, _ = _sched_and_diffusion(golden, 16)
    (H, W), (h, w), windows = case["size"], case["window"], case["windows"]
    for m in (16, 0):
        d.train_weights = None
        d.train_crop, d.train_crop_margin = (h, w), m
        l_crop, g_crop = _crop_step(net, d, case["x_start"], case["x_orig"], case["noise"], case["t"], 1, windows)
        d.train_crop = None
        parts = []
        for b, origin in enumerate(windows):
            ylo, yhi, xlo, xhi = rect_of(origin, (H, W), (h, w), m)
            wmap = torch.zeros(H, W)
            wmap[origin[0] + ylo:origin[0] + yhi, origin[1] + xlo:origin[1] + xhi] = 1
            d.train_weights = [None, wmap.to(DEV), None]
            sl = slice(b, b + 1)
            l, g = _step(net, d, case["x_start"][sl], case["x_orig"][sl], case["noise_full"][sl], case["t"][sl], 1)
            parts.append((float(wmap.sum()), l, g))
        l_full, g_full = combine_by_area(parts)
        diff = {k: rel_l2(g_crop[k], g_full[k]) for k in g_full}
        print(f"[margin {m}] loss {abs(l_crop - l_full) / abs(l_full):.1e}; gradients {min(diff.values()):.1e} .. "
              f"{max(diff.values()):.1e}")
        assert len(diff) == 52
        if m == 16:
            assert abs(l_crop - l_full) < 4e-4 * abs(l_full)
            for k, e in diff.items():
                assert e < 4e-4, (k, e)
        else:
            assert max(diff.values()) > 1e-2


# ---- 7 / 8: nothing changes when off, or at a scale the crop does not cut ------------------------------------------------------------
def _recorded(golden, how, x_start, x_orig, noise, t, s, monkeypatch):
    """One plain 7x12 step on a fresh diffusion object (train_step_util.recorded_step) during which the two new entries refuse
    to run.  how = 'touched': the object first ran a CROPPED step, then had train_crop set back to None; 'larger': train_crop
    is set, and not smaller than the scale."""
    net, d, _, _ = _sched_and_diffusion(golden, 16)
    if how == "touched":
        d.train_crop, d.train_crop_margin = (5, 8), 1
        cropped, _ = _crop_step(net, d, x_start, x_orig, hash_randn((2, 3, 5, 8), 601), t, s, [(0, 1), (2, 4)])
        d.train_crop = None
    elif how == "larger":
        d.train_crop, d.train_crop_margin = (7, 16), 3
    rec = recorded_step(monkeypatch, net, d, x_start, x_orig, noise, t, s, (Q_NAME, L_NAME),
                        "a crop-training kernel ran on a step that is not cropped")
    if how == "touched":
        assert cropped != rec["loss"]                                          # (the cropped step was another step)
    return rec


@pytest.mark.parametrize("s", [0, 2])
def test_off_is_the_untouched_step(golden, monkeypatch, s):
    """train_crop = None, set explicitly after a cropped step (7), and train_crop = (7, 16) on a 7x12 scale (8), against a
    diffusion object whose attributes were never touched.  The rule of tests/test_gpu_train_mask.py::
    test_off_is_the_untouched_step: neither new entry is called; the loss, x_noisy, the network's output and the gradient handed
    to its backward are bit-equal; the flat gradient buffer, which the backward kernels accumulate with fp32 atomics in an
    order that varies run to run, is held to 2e-6 rel-L2 per tensor."""
    x_start, x_orig, noise, t = _inputs(2, 7, 12, 600)
    a = _recorded(golden, "untouched", x_start, x_orig, noise, t, s, monkeypatch)
    for how in ("touched", "larger"):
        other = _recorded(golden, how, x_start, x_orig, noise, t, s, monkeypatch)
        assert other["loss"] == a["loss"], how
        for k in ("x_noisy", "eps", "grad_eps"):
            assert torch.equal(other[k], a[k]), (how, k)
        for n, off in a["named"].items():
            sl = slice(off, off + a["numel"][n])
            assert rel_l2(other["flat_grads"][sl], a["flat_grads"][sl]) < 2e-6, (how, n)
    assert float(a["flat_grads"].abs().sum()) > 0


def test_which_entries_a_step_calls(golden, monkeypatch):
    """Counted on the library: a scale not larger than the crop calls today's two entries, a cropped one the two new ones."""
    net, d, _, _ = _sched_and_diffusion(golden, 16)
    d.train_crop, d.train_crop_margin = (7, 16), 3
    x_start, x_orig, noise, t = _inputs(2, 7, 12, 600)
    with monkeypatch.context() as m:
        calls = count_entries(m, ("sinddm_q_sample", "sinddm_l1_loss_fwd_bwd", Q_NAME, L_NAME))
        _step(net, d, x_start, x_orig, noise, t, 1)
        assert calls == {"sinddm_q_sample": 1, "sinddm_l1_loss_fwd_bwd": 1}
        calls.clear()
        d.train_crop, d.train_crop_margin = (7, 8), 1
        _crop_step(net, d, x_start, x_orig, hash_randn((2, 3, 7, 8), 602), t, 1, [(0, 0), (0, 4)])
        assert calls == {Q_NAME: 1, L_NAME: 1}


# ---- 9: the trainer ---------------------------------------------------------------------------------------------------------------
def _trainer(golden, tmp_path, **kw):
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
    tr = MultiscaleTrainer(d, folder=folder, n_scales=n, scale_factor=meta["scale_factor"],
                           image_sizes=[tuple(v) for v in meta["sizes"]], train_batch_size=2, train_lr=1e-3, train_num_steps=2,
                           gradient_accumulate_every=1, save_and_sample_every=10 ** 9, results_folder=str(tmp_path / "res"),
                           device=DEV, train_crop=(40, 48), train_crop_margin=16, **kw)
    return net, d, tr, n


def test_trainer_trains_on_crops(golden, tmp_path):
    """MultiscaleTrainer(train_crop=(40, 48), train_crop_margin=16) over the C1 pyramid of tests/golden/balloons.png: two
    optimizer steps (the coarsest and the finest scale, through scale_fn) give finite losses and move the parameters; the
    network saw 40x48 windows of the 94x126 finest scale; the EMA copy keeps train_crop = None."""
    net, d, tr, n = _trainer(golden, tmp_path)
    assert tr.model.train_crop == (40, 48) and tr.model.train_crop_margin == 16
    assert tr.ema_model.train_crop is None and tr.ema_model.train_crop_margin == 0
    seq = [0, n - 1]
    tr.scale_fn = lambda step: seq[step]
    losses, shapes, before = [], [], net.flat_params.detach().clone()
    forward = d.forward
    d.forward = lambda x, s, *a, **k: losses.append(forward(x, s, *a, **k)) or losses[-1]
    h = net.register_forward_hook(lambda mod, args, out: shapes.append(tuple(args[0].shape)))
    try:
        tr.train()
    finally:
        h.remove()
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(bool(torch.isfinite(l)) and float(l) > 0 for l in losses)
    assert tuple(d.image_sizes[n - 1]) == (94, 126) and shapes == [(2, 3, 40, 48), (2, 3, 40, 48)]
    assert bool(torch.isfinite(net.flat_params).all()) and not torch.equal(net.flat_params, before)


def test_trainer_raises_when_no_window_holds_weight(golden, tmp_path):
    """A train_mask whose hole swallows the one window a forced crop_fn ever returns: p_losses asks crop_fn 1 + 16 times, then
    raises SinddmError -- before anything is launched (the parameters have not moved)."""
    from sinddm_amd import _lib
    from sinddm_amd.train_step import CROP_REDRAWS
    valid = torch.ones(94, 126)
    valid[:44, :52] = 0                                                        # the window at (0, 0) and a little more
    net, d, tr, n = _trainer(golden, tmp_path, train_mask=valid)
    asked = []
    d.crop_fn = lambda step, s, B: asked.append((step, s, B)) or torch.zeros(B, 2, dtype=torch.long)
    tr.scale_fn = lambda step: n - 1
    before = net.flat_params.detach().clone()
    with pytest.raises(_lib.SinddmError, match="no weight"):
        tr.train()
    assert asked == [(0, n - 1, 2)] * (1 + CROP_REDRAWS)
    assert torch.equal(net.flat_params, before)
