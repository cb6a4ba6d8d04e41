"""Cost of tileable training (`train_tile`) on the C2 training step, and of the fused x_noisy kernel.

    python tools/tile_train_time.py step    --train_tile none|x|y|xy [--scales 0 1 2 3 4] [--batch 32] [--steps 5]
    python tools/tile_train_time.py qsample --train_tile x|y|xy      [--scale 4] [--batch 32] [--iters 200]

ONE configuration per process (alternate fresh processes of the configurations on one box).  Prints one JSON line.
  step     MultiScaleGaussianDiffusion.forward + backward + fused Adam per scale of C2 (dim 160), as tools/train_bench.py times
           it: two warm-up steps, `--steps` timed ones, host clocks around device-synchronised loops.  With a wrapped axis the
           network runs on the image extended by 16 pixels on both sides of it: `pixels_ratio` is (H+2hy)(W+2hx)/(HW).
  qsample  sinddm_q_sample_wrap (one pass) against sinddm_q_sample + sinddm_wrap_halo (two passes, what it replaces) on the
           scale's (batch,3,H,W) tensors with x_orig, into preallocated buffers: device events around `--iters` back-to-back
           calls of each, three rounds alternating.  `*_enqueue_us` is the host's time to enqueue one call: where it is not
           well below the device figure, the device figure measures the host.  The same tensors are read every call (at batch
           32 they stay in the last-level cache): `--batch 256` is the run that has to go to HBM."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

PAIR = {"none": (False, False), "x": (False, True), "y": (True, False), "xy": (True, True)}


def step_times(args, d, net, dev):
    from sinddm_amd.optim import FusedAdam
    opt = FusedAdam(net, lr=1e-3)
    out = []
    for s in args.scales:
        H, W = d.image_sizes[s]
        torch.manual_seed(11 + s)
        img = torch.randn(args.batch, 3, H, W, device=dev).clamp(-1, 1)
        data = (img, img.clone())

        def run(n):
            for _ in range(n):
                loss = d(data, s)
                loss.backward()
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            return float(loss.detach())

        run(2)
        t0 = time.perf_counter()
        loss = run(args.steps)
        dt = (time.perf_counter() - t0) / args.steps
        hy, hx = (16 if d.train_tile[0] else 0), (16 if d.train_tile[1] else 0)
        out.append({"scale": s, "size_hw": [H, W], "ms_per_step": round(1e3 * dt, 2),
                    "pixels_ratio": round((H + 2 * hy) * (W + 2 * hx) / (H * W), 3), "loss": round(loss, 5)})
    return out


def qsample_times(args, d, dev):
    from sinddm_amd import _lib
    from sinddm_amd.synth import hash_randn
    lib = _lib.load()
    s = args.scale
    H, W = d.image_sizes[s]
    B = args.batch
    hy, hx = (16 if d.train_tile[0] else 0), (16 if d.train_tile[1] else 0)
    x0, xo, nz = ((hash_randn((1, 3, H, W), 5 + k) * 0.5).to(dev).repeat(B, 1, 1, 1).contiguous() for k in range(3))
    t = torch.randint(0, d.num_timesteps, (B,), device=dev)
    gam = d.gammas[s - 1].reshape(-1).contiguous()
    assert torch.equal(d._q_sample_impl(x0, t, 0, nz, x_orig=xo, gamma_row=gam, halo=(hy, hx)),
                       d._wrap_pad(d._q_sample_impl(x0, t, 0, nz, x_orig=xo, gamma_row=gam), hy, hx))
    # the entry points themselves on preallocated buffers: as little host work per call as ctypes allows
    out = torch.empty_like(x0)
    ext = torch.empty((B, 3, H + 2 * hy, W + 2 * hx), device=dev)
    st = _lib.stream_ptr(dev)
    P = {k: _lib.ptr(v) for k, v in dict(x0=x0, xo=xo, nz=nz, out=out, ext=ext, a=d.sqrt_alphas_cumprod,
                                          b=d.sqrt_one_minus_alphas_cumprod, g=gam, t=t).items()}

    def fused():
        lib.sinddm_q_sample_wrap(P["x0"], P["xo"], P["nz"], P["ext"], P["a"], P["b"], P["g"], P["t"], 0, B, 3, H, W, hy, hx, st)

    def two():
        lib.sinddm_q_sample(P["x0"], P["xo"], P["nz"], P["out"], P["a"], P["b"], P["g"], P["t"], 0, B, 3 * H * W, st)
        lib.sinddm_wrap_halo(P["ext"], P["out"], B * 3, H, W, hy, hx, st)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        a.record()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        host = time.perf_counter() - t0                         # time to ENQUEUE: the clock stops before the synchronise
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters * 1e3, host / args.iters * 1e6      # microseconds per call: device, host

    rounds = [(timed(fused), timed(two)) for _ in range(3)]
    med = lambda k, i: statistics.median(r[k][i] for r in rounds)
    return {"scale": s, "size_hw": [H, W], "halo": [hy, hx], "MB_per_tensor": round(x0.numel() * 4 / 2 ** 20, 1),
            "fused_us": [round(r[0][0], 2) for r in rounds], "two_pass_us": [round(r[1][0], 2) for r in rounds],
            "fused_enqueue_us": round(med(0, 1), 2), "two_pass_enqueue_us": round(med(1, 1), 2),
            "ratio_median": round(med(0, 0) / med(1, 0), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("step", "qsample"))
    ap.add_argument("--train_tile", choices=tuple(PAIR), required=True)
    ap.add_argument("--scales", type=int, nargs="+", default=[0, 1, 2, 3, 4])
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        raise SystemExit("tile_train_time.py measures on the GPU: no device found")
    from sinddm_amd.configs import build_diffusion
    dev = torch.device("cuda:0")
    net, d = build_diffusion("C2", 160, dev)
    d.train_tile = PAIR[args.train_tile]
    rec = {"tool": "tile_train_time", "what": args.what, "config": "C2", "dim": 160, "batch": args.batch,
           "train_tile": args.train_tile, "device": torch.cuda.get_device_name(0)}
    if args.what == "step":
        rec["steps"] = args.steps
        rec["scales"] = step_times(args, d, net, dev)
    else:
        if args.train_tile == "none":
            raise SystemExit("qsample needs a wrapped axis")
        rec["iters"] = args.iters
        rec.update(qsample_times(args, d, dev))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
