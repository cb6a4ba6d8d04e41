#!/usr/bin/env python3
"""Cost of masked training (MultiScaleGaussianDiffusion.train_weights) on C2 (dim 160) at batch 32.

    train_mask_time.py step S N [--mask]   ms per training step (forward + backward + fused Adam) at pyramid scale S, two warm-up
                                           and N timed steps: tools/train_bench.py's loop, with --mask under a weight map whose
                                           hole (a sixth of the height by a fifth of the width) is grown by 16 pixels
    train_mask_time.py kernel              us per call of sinddm_l1_loss_weighted_fwd_bwd beside sinddm_l1_loss_crop_fwd_bwd and
                                           sinddm_l1_loss_fwd_bwd on the tensors of scales 4 and 0, 200 back-to-back calls
                                           between two device events, three rounds alternating

One configuration per fresh process; alternate the processes on one box."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sinddm_amd import _lib                                                     # noqa: E402
from sinddm_amd.configs import build_diffusion                                  # noqa: E402
from sinddm_amd.functions import train_weight_pyramid                           # noqa: E402
from sinddm_amd.optim import FusedAdam                                          # noqa: E402

dev = torch.device("cuda:0")


def hole_map(H, W, grow=16):
    valid = torch.ones(H, W)
    valid[H // 3:H // 3 + H // 6, W // 4:W // 4 + W // 5] = 0
    return train_weight_pyramid(valid, [(H, W)], grow=grow)[0].to(dev)


def step(s, n, mask):
    net, d = build_diffusion("C2", 160, dev)
    opt = FusedAdam(net, lr=1e-3)
    H, W = d.image_sizes[s]
    if mask:
        d.train_weights = [None] * s + [hole_map(H, W)]
    img = torch.randn(32, 3, H, W, device=dev).clamp(-1, 1)
    data = (img, img.clone())
    for _ in range(2):
        loss = d(data, s); loss.backward(); opt.step(); opt.zero_grad()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        loss = d(data, s); loss.backward(); opt.step(); opt.zero_grad()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
    print(json.dumps(dict(scale=s, H=H, W=W, batch=32, mask=bool(mask), ms_per_step=round(dt * 1e3, 3), loss=float(loss),
                          valid_share=round(float(d.train_weights[s].mean()), 3) if mask else 1.0)))


def kernel():
    lib = _lib.load()
    _, d = build_diffusion("C2", 160, dev)
    st = _lib.stream_ptr(dev)
    for s in (4, 0):
        H, W = d.image_sizes[s]
        B = 32
        noise, eps = torch.randn(B, 3, H, W, device=dev), torch.randn(B, 3, H, W, device=dev)
        w = hole_map(H, W)
        inv = 1.0 / (B * 3 * float(w.double().sum()))
        g, loss = torch.empty_like(eps), torch.zeros((), device=dev)
        p = _lib.ptr
        calls = {
            "weighted": lambda: lib.sinddm_l1_loss_weighted_fwd_bwd(p(noise), p(eps), p(w), p(loss), p(g), B, 3, H, W, 0, 0, inv,
                                                                    1.0, st),
            "crop": lambda: lib.sinddm_l1_loss_crop_fwd_bwd(p(noise), p(eps), p(loss), p(g), B * 3, H, W, 0, 0, 1.0, st),
            "plain": lambda: lib.sinddm_l1_loss_fwd_bwd(p(noise), p(eps), p(loss), p(g), noise.numel(), 1.0, st),
        }
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
        print(json.dumps(dict(scale=s, H=H, W=W, batch=B, us_per_call=out)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        kernel()
    else:
        step(int(sys.argv[2]), int(sys.argv[3]), "--mask" in sys.argv)
