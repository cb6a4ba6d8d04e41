"""Shared by tests/test_crop_train_host.py and tests/test_gpu_crop_train.py: crop training restated, in float64 and in numpy.

Crop training (MultiScaleGaussianDiffusion.train_crop): sample b of a step sees the (h,w) window of the (H,W) image
at (y0_b, x0_b); its valid rectangle V_b is the window minus `margin` rows / columns along every side that is not an image
border, and the loss is sum_b sum_c sum_{p in V_b} w(p) e / (C sum_b sum_{p in V_b} w(p)).  Everything here is written from
that sentence, in plain Python integers, numpy and the oracle's own functions; nothing calls sinddm_amd.functions, which is
what the tests compare against."""
import numpy as np
import torch

from oracle import sinddm_oracle as O
from sinddm_amd.synth import hash_randn, he_state_dict
from tile_train_util import autograd_in, sched_in
from train_mask_util import weighted_p_losses_autograd

# the (H, h, m) triples of DESIGN.md 4's coverage statement
TRIPLES = [(186, 96, 16), (186, 96, 0), (248, 128, 16), (1024, 256, 16), (64, 48, 16), (50, 40, 16), (100, 34, 16), (12, 8, 2),
           (13, 8, 3), (9, 8, 0), (9, 8, 3), (40, 39, 16)]


def valid_range(o, n, k, m):
    """The half-open valid range, in IMAGE coordinates, of a k-pixel window at origin o on an axis of n pixels."""
    if k == n:
        return 0, n
    return (o if o == 0 else o + m), (o + k if o == n - k else o + k - m)


def rect_of(origin, size, window, m):
    """(y_lo, y_hi, x_lo, x_hi) in WINDOW coordinates."""
    out = []
    for o, n, k in zip(origin, size, window):
        lo, hi = valid_range(int(o), int(n), int(k), m)
        out += [lo - int(o), hi - int(o)]
    return tuple(out)


def coverage(n, k, m, clamped=True):
    """How many of the draws supervise each pixel of an axis, by exhaustive enumeration: the clamped draw (o' over
    -(L-1) .. n - k + (L-1), o = clamp(o', 0, n - k)) or the uniform one (o over 0 .. n - k)."""
    L = k - 2 * m
    draws = range(-(L - 1), n - k + (L - 1) + 1) if clamped else range(0, n - k + 1)
    hits = np.zeros(n, np.int64)
    for o in draws:
        lo, hi = valid_range(min(max(o, 0), n - k), n, k, m)
        hits[lo:hi] += 1
    return hits


def brute_norm(windows, rects, wmap=None):
    """sum_b sum_{p in V_b} w(p), pixel by pixel in float64."""
    tot = 0.0
    for (y0, x0), (ylo, yhi, xlo, xhi) in zip(windows, rects):
        for y in range(ylo, yhi):
            for x in range(xlo, xhi):
                tot += 1.0 if wmap is None else float(np.float64(wmap[y0 + y, x0 + x]))
    return tot


def window_mask(B, window, rects, windows=None, wmap=None, dtype=torch.float64):
    """(B,1,h,w): w(p) inside each sample's rectangle, 0 outside."""
    h, w = window
    out = torch.zeros(B, 1, h, w, dtype=dtype)
    for b, (ylo, yhi, xlo, xhi) in enumerate(rects):
        if wmap is None:
            out[b, 0, ylo:yhi, xlo:xhi] = 1
        else:
            y0, x0 = windows[b]
            out[b, 0, ylo:yhi, xlo:xhi] = wmap[y0 + ylo:y0 + yhi, x0 + xlo:x0 + xhi].to(dtype)
    return out


def gather_windows(x, windows, window):
    h, w = window
    return torch.stack([x[b, :, y0:y0 + h, x0:x0 + w] for b, (y0, x0) in enumerate(windows)])


def place_windows(full, small, windows):
    """A copy of the (B,C,H,W) tensor `full` whose windows hold `small` (B,C,h,w)."""
    out = full.clone()
    h, w = small.shape[-2:]
    for b, (y0, x0) in enumerate(windows):
        out[b, :, y0:y0 + h, x0:x0 + w] = small[b]
    return out


def crop_p_losses(sched, sd, x_start, t, s, noise, x_orig, mask, windows, loss_type="l1"):
    """The cropped step: the oracle's x_noisy and network on the windows, the weighted sum over `mask` (B,1,h,w) / (C sum)."""
    window = noise.shape[-2:]
    xs = gather_windows(x_start, windows, window)
    xo = gather_windows(x_orig, windows, window) if x_orig is not None else None
    eps = O.net_forward(sd, O.p_losses_inputs(sched, xs, t, s, noise, xo), t, s)
    if loss_type == "l1":
        e = (noise - eps).abs()
    elif loss_type == "l2":
        e = (noise - eps) ** 2
    elif loss_type == "l1_pred_img":
        if int(s) > 0 and int(t[0]) > 0:
            g = O.extract(sched["gammas"][s - 1].reshape(-1), t - 1)
            target = g * xs + (1 - g) * xo
        else:
            target = xo if int(s) > 0 else xs
        e = (target - eps).abs()
    else:
        raise NotImplementedError(loss_type)
    return (e * mask).sum() / (e.shape[1] * mask.sum())


def crop_p_losses_autograd(sched, sd, x_start, x_orig, t, s, noise, mask, windows, loss_type="l1", dtype=torch.float64):
    """crop_p_losses under autograd in `dtype`: (loss as a float, {name: grad})."""
    sc = sched_in(sched, dtype)
    if x_orig is None:
        fn = lambda p, xs, nz, mk: crop_p_losses(sc, p, xs, t, s, nz, None, mk, windows, loss_type)
        val, g = autograd_in(dtype, fn, sd, x_start, noise, mask)
    else:
        fn = lambda p, xs, nz, mk, xo: crop_p_losses(sc, p, xs, t, s, nz, xo, mk, windows, loss_type)
        val, g = autograd_in(dtype, fn, sd, x_start, noise, mask, x_orig)
    return float(val), g


def combine_by_area(parts):
    """[(area, loss, {name: grad})] of B = 1 steps -> the loss and gradients of the step that normalises by the total area."""
    tot = float(sum(a for a, _, _ in parts))
    loss = sum(a * l for a, l, _ in parts) / tot
    grads = {k: sum((a / tot) * g[k].to(torch.float64) for a, _, g in parts) for k in parts[0][2]}
    return loss, grads


def statement_case(golden):
    """The set-up of the receptive-radius statement: dim 16, He-normal weights, full image 48x64 at scale 1 (x_orig takes
    part), window 40x44, B = 2 with origins (0, 12) -- one closed side -- and (8, 20) -- two: the bottom and the right."""
    meta = golden("g11_img_scales.json")["C1"]
    sched = O.make_schedule(meta["T"], meta["n_scales"], meta["rescale_losses"], 1, train_full_t=True)
    sd = he_state_dict(16)
    B, H, W, h, w = 2, 48, 64, 40, 44
    x_start = hash_randn((B, 3, H, W), 911).mul(0.5).clamp(-1, 1)
    x_orig = hash_randn((B, 3, H, W), 912).mul(0.5).clamp(-1, 1)
    noise = hash_randn((B, 3, h, w), 913)                                     # window size
    noise_full = hash_randn((B, 3, H, W), 914)                                # what the full-image steps hold outside the windows
    t = torch.tensor([7, 31])
    windows = [(0, 12), (8, 20)]
    return dict(sched=sched, sd=sd, size=(H, W), window=(h, w), x_start=x_start, x_orig=x_orig, noise=noise,
                noise_full=place_windows(noise_full, noise, windows), t=t, windows=windows)


def statement_full_steps_f64(case, m):
    """The two B = 1 full-image masked steps (maps 1_{V_b}) in float64, combined by area."""
    parts = []
    for b, origin in enumerate(case["windows"]):
        ylo, yhi, xlo, xhi = rect_of(origin, case["size"], case["window"], m)
        wmap = torch.zeros(case["size"])
        wmap[origin[0] + ylo:origin[0] + yhi, origin[1] + xlo:origin[1] + xhi] = 1
        sl = slice(b, b + 1)
        l, g = weighted_p_losses_autograd(case["sched"], case["sd"], case["x_start"][sl], case["x_orig"][sl], case["t"][sl], 1,
                                          case["noise_full"][sl], wmap)
        parts.append((float(wmap.sum()), l, g))
    return combine_by_area(parts)


def l1_rect_reference(noise, eps, wmap, windows, rects, inv_norm, grad_scale):
    """What sinddm_l1_loss_rect_fwd_bwd has to give for CPU tensors noise / eps (B,C,h,w): (the loss as the float64 sum over
    the rectangle elements with w > 0, times float64(float32(inv_norm)); the gradient in fp32 numpy arithmetic,
    ((sign * inv_norm) * grad_scale) * w in that order, 0 outside the rectangles and where w == 0), and the boolean `on`."""
    B, C, h, w = noise.shape
    wb = window_mask(B, (h, w), rects, windows, wmap, dtype=torch.float32).numpy()
    inside = window_mask(B, (h, w), rects, dtype=torch.float32).numpy() > 0
    on = np.broadcast_to(inside & (wb > 0), noise.shape)
    wn = np.broadcast_to(wb, noise.shape).astype(np.float32)
    inv32, gs32 = np.float32(inv_norm), np.float32(grad_scale)
    with np.errstate(invalid="ignore"):
        d = noise.numpy() - eps.numpy()
    contrib = np.where(on, np.abs(d.astype(np.float64)) * wn.astype(np.float64), 0.0)
    loss = float(contrib.sum() * np.float64(inv32))
    sign = np.where(d > 0, np.float32(-1), np.where(d < 0, np.float32(1), np.float32(0))).astype(np.float32)
    with np.errstate(invalid="ignore"):
        g = np.where(on, ((sign * inv32) * gs32) * wn, np.float32(0)).astype(np.float32)
    return loss, g, on
