#!/usr/bin/env python3
"""One C2 pyramid with patch refinement, exhaustive or windowed, in a fresh process: wall time and what the samples copy.

    python tools/refine_pyramid_time.py [--radius R] [--scales 2 4] [--patch 7] [--iters 1] [--steps 8] [--off]

dim 160, synthetic closed-form weights, batch 16, seeds 0 ... 15, the C2 pyramid of tests/golden/balloons.png (48x64 ...
186x248), `sample_steps` = --steps per scale.  The process runs `sample_scales` twice and reports the wall time of the second
call, then `patch_report` (P = --patch, exhaustive) of the finest batch, and with --radius the share of the finest scale's
queries whose windowed winner is the exhaustive one (a third, untimed run that searches the same input both ways).
Prints one JSON line.  Run it several times, alternating the variants: every process is one sample of the wall time."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--radius", type=int, default=None)
    ap.add_argument("--scales", type=int, nargs=2, default=[2, 4])
    ap.add_argument("--patch", type=int, default=7)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--off", action="store_true", help="no refinement at all")
    args = ap.parse_args()
    from sinddm_amd.configs import CONFIGS, build_diffusion
    from sinddm_amd.trainer import MultiscaleTrainer
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = CONFIGS["C2"]
    n = len(cfg["sizes"])
    src = Image.open(os.path.join(REPO, "tests", "golden", "balloons.png")).convert("RGB")
    with tempfile.TemporaryDirectory(prefix="sinddm_refine_time_") as tmp:
        pyramid = [src.resize(tuple(size), Image.LANCZOS) for size in cfg["sizes"]]
        for i, img in enumerate(pyramid):
            os.makedirs(os.path.join(tmp, f"scale_{i}"))
            img.save(os.path.join(tmp, f"scale_{i}", "balloons.png"))
            if i:
                os.makedirs(os.path.join(tmp, f"scale_{i}_recon"))
                pyramid[i - 1].resize(tuple(cfg["sizes"][i]), Image.BILINEAR).save(os.path.join(tmp, f"scale_{i}_recon", "balloons.png"))
        net, d = build_diffusion("C2", 160, dev)
        tr = MultiscaleTrainer(d, folder=tmp + "/", n_scales=n, scale_factor=cfg["scale_factor"], image_sizes=cfg["sizes"],
                               train_batch_size=16, train_lr=2e-5, train_num_steps=1, gradient_accumulate_every=1,
                               step_start_ema=2000, update_ema_every=10, save_and_sample_every=10 ** 9, avg_window=100,
                               results_folder=os.path.join(tmp, "results"), device=dev)
        em = tr.ema_model
        em.sample_steps = args.steps
        opt = None
        if not args.off:
            opt = dict(iters=args.iters, patch=args.patch, scales=tuple(args.scales))
            if args.radius is not None:
                opt["radius"] = args.radius
        kw = dict(batch_size=16, save_images=False, seeds=list(range(16)))
        if opt is not None:
            kw["patch_refine"] = opt
        tr.sample_scales(**kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tr.sample_scales(**kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        rep = tr.evaluate(samples=out, patch=args.patch)
        rec = {"variant": "off" if opt is None else "exhaustive" if args.radius is None else f"radius {args.radius}",
               "scales": list(args.scales), "patch": args.patch, "iters": args.iters, "sample_steps": args.steps,
               "ms": round(ms, 2), "fidelity": round(rep["fidelity_mean"], 4), "coherence": round(rep["coherence_mean"], 4),
               "coverage": round(rep["coverage_mean"], 4)}
        if opt is not None and args.radius is not None:
            shares, refine = {}, tr.refine

            def both(cur, **rkw):                      # the same input searched both ways, per windowed scale
                res = refine(cur, **rkw)
                if rkw.get("prior") is not None:
                    full = refine(cur, **{k: v for k, v in rkw.items() if k not in ("radius", "prior")})
                    shares[int(rkw["scale"])] = round(float((full[-1] == res[-1]).all(dim=1).float().mean()), 4)
                return res

            tr.refine = both
            tr.sample_scales(**kw)
            rec["winners_equal_exhaustive"] = shares
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
