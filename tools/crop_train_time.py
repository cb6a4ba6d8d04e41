#!/usr/bin/env python3
"""Cost of crop training (MultiScaleGaussianDiffusion.train_crop) on C2 (dim 160) at batch 32.

    crop_train_time.py step S N [--crop H W] [--margin M]
        ms per training step (forward + backward + fused Adam) at pyramid scale S, two warm-up and N timed steps:
        tools/train_bench.py's loop.  With --crop the windows come from the clamped draw (functions.crop_windows) through
        crop_fn, which also counts the supervised pixel-samples (the area of the valid rectangles) of the timed steps.
    crop_train_time.py kernel
        us per call of sinddm_q_sample_crop beside sinddm_q_sample, and of sinddm_l1_loss_rect_fwd_bwd beside
        sinddm_l1_loss_weighted_fwd_bwd, on equal element counts (32 x 3 x 96 x 96 and 32 x 3 x 128 x 128 windows of the
        186 x 248 scale against full tensors of the window's size), 200 back-to-back calls between two device events, three
        rounds alternating
    crop_train_time.py route
        the 3x3 route (sinddm_debug_train_path) of the training launches at 96 x 96, 128 x 128 and 186 x 248

One configuration per fresh process; alternate the processes on one box."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sinddm_amd import _lib                                                     # noqa: E402
from sinddm_amd import functions as F                                           # noqa: E402
from sinddm_amd.configs import build_diffusion                                  # noqa: E402
from sinddm_amd.optim import FusedAdam                                          # noqa: E402

dev = torch.device("cuda:0")
B = 32


def step(s, n, crop, margin):
    net, d = build_diffusion("C2", 160, dev)
    opt = FusedAdam(net, lr=1e-3)
    H, W = d.image_sizes[s]
    seen = []
    if crop is not None:
        gen = torch.Generator().manual_seed(1)
        d.train_crop, d.train_crop_margin = crop, margin

        def crop_fn(step_, s_, b):
            win = F.crop_windows(gen, b, (H, W), crop, margin)
            seen.append(F.crop_norm(win, F.crop_rects(win, (H, W), crop, margin)))
            return win
        d.crop_fn = crop_fn
    img = torch.randn(B, 3, H, W, device=dev).clamp(-1, 1)
    data = (img, img.clone())
    for _ in range(2):
        loss = d(data, s); loss.backward(); opt.step(); opt.zero_grad()
    del seen[:]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        loss = d(data, s); loss.backward(); opt.step(); opt.zero_grad()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
    pix = sum(seen) / len(seen) if seen else float(B * H * W)
    print(json.dumps(dict(scale=s, H=H, W=W, batch=B, crop=crop, margin=margin, ms_per_step=round(dt * 1e3, 3),
                          supervised_pixel_samples=round(pix), ms_per_Mpix=round(dt * 1e3 / (pix / 1e6), 2), loss=float(loss))))


def _time(calls):
    out = {k: [] for k in calls}
    for _ in range(3):
        for name, fn in calls.items():
            for _ in range(10):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(200):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(round(a.elapsed_time(b) * 1e3 / 200, 2))
    return out


def kernel():
    lib = _lib.load()
    _, d = build_diffusion("C2", 160, dev)
    st, p = _lib.stream_ptr(dev), _lib.ptr
    H, W = d.image_sizes[4]
    tabs = (p(d.sqrt_alphas_cumprod), p(d.sqrt_one_minus_alphas_cumprod))
    gam = d.gammas[3].reshape(-1).contiguous()
    t = torch.randint(0, 50, (B,), device=dev)
    x0, xo = torch.randn(B, 3, H, W, device=dev), torch.randn(B, 3, H, W, device=dev)
    wmap = torch.rand(H, W, device=dev)
    for h, w, m in ((96, 96, 16), (128, 128, 16)):
        gen = torch.Generator().manual_seed(1)
        win_h = F.crop_windows(gen, B, (H, W), (h, w), m)
        rect_h = F.crop_rects(win_h, (H, W), (h, w), m)
        win, rect = win_h.to(dev, torch.int32).contiguous(), rect_h.to(dev, torch.int32).contiguous()
        nz, out = torch.randn(B, 3, h, w, device=dev), torch.empty(B, 3, h, w, device=dev)
        s0, so = torch.randn(B, 3, h, w, device=dev), torch.randn(B, 3, h, w, device=dev)      # full tensors of the window's size
        eps, g, loss = torch.randn(B, 3, h, w, device=dev), torch.empty(B, 3, h, w, device=dev), torch.zeros((), device=dev)
        wsmall = torch.rand(h, w, device=dev)
        inv = 1.0 / (3 * F.crop_norm(win_h, rect_h))
        calls = {
            "q_sample_crop": lambda: lib.sinddm_q_sample_crop(p(x0), p(xo), p(nz), p(out), tabs[0], tabs[1], p(gam), p(t), 0, p(win),
                                                              B, 3, H, W, h, w, st),
            "q_sample": lambda: lib.sinddm_q_sample(p(s0), p(so), p(nz), p(out), tabs[0], tabs[1], p(gam), p(t), 0, B, 3 * h * w,
                                                    st),
            "l1_rect": lambda: lib.sinddm_l1_loss_rect_fwd_bwd(p(nz), p(eps), None, None, p(rect), p(loss), p(g), B, 3, h, w, 0, 0,
                                                               inv, 1.0, st),
            "l1_rect_map": lambda: lib.sinddm_l1_loss_rect_fwd_bwd(p(nz), p(eps), p(wmap), p(win), p(rect), p(loss), p(g), B, 3, h,
                                                                   w, H, W, inv, 1.0, st),
            "l1_weighted": lambda: lib.sinddm_l1_loss_weighted_fwd_bwd(p(nz), p(eps), p(wsmall), p(loss), p(g), B, 3, h, w, 0, 0,
                                                                       inv, 1.0, st),
        }
        print(json.dumps(dict(window=(h, w), of=(H, W), batch=B, margin=m, us_per_call=_time(calls))))


def route():
    lib = _lib.load()
    print(json.dumps({f"{h}x{w}": lib.sinddm_debug_train_path(160, B, h, w) for h, w in ((96, 96), (128, 128), (186, 248))}))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "step"
    if mode == "kernel":
        kernel()
    elif mode == "route":
        route()
    else:
        crop = None
        if "--crop" in sys.argv:
            i = sys.argv.index("--crop")
            crop = (int(sys.argv[i + 1]), int(sys.argv[i + 2]))
        margin = int(sys.argv[sys.argv.index("--margin") + 1]) if "--margin" in sys.argv else 0
        step(int(sys.argv[2]), int(sys.argv[3]), crop, margin)
