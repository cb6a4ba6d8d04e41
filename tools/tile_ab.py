"""Cost of tileable sampling: per-scale time of one full sample with `tile` off, on x, and on both axes.

    python tools/tile_ab.py [--config C2] [--dim 160] [--batch 16] [--runs 3] [--out FILE.json]

A wrapped axis carries a halo of SINDDM_TILE_HALO = 16 pixels on both sides, so the network runs on (H+32)(W+32) pixels
instead of HW (both axes) or H(W+32) (x only): the area ratio is the cost one expects where the GPU is busy; where a scale
is launch-bound the extension can be cheaper than that, and a change of kernel path or of the two-stream split can make
it dearer.  The tool prints the measured ratio next to the area ratio.

Same process, same library, closed-form weights; one warm-up sample of each variant, then `--runs` timed samples of each,
interleaved.  Times are host clocks around device-synchronised scale calls (MultiScaleGaussianDiffusion.sample /
sample_via_scale: upsample + re-noise + every reverse step of the scale).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("off", (False, False)), ("x", (False, True)), ("xy", (True, True)))


def timed_sample(d, batch, tile):
    """One sample over the full pyramid; returns seconds per scale."""
    per_scale = []
    img = None
    with d.sampling(tile=tile):
        for s in range(d.n_scales):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            img = d.sample(batch_size=batch, s=0) if s == 0 else d.sample_via_scale(batch, img, s=s)
            torch.cuda.synchronize()
            per_scale.append(time.perf_counter() - t0)
            assert tuple(img.shape[2:]) == tuple(d.image_sizes[s]) and bool(torch.isfinite(img).all())
    return per_scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dim", type=int, default=160)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tile_ab.py measures on the GPU: no device found")
    from sinddm_amd import _lib
    from sinddm_amd.configs import build_diffusion
    dev = torch.device("cuda:0")
    net, d = build_diffusion(args.config, args.dim, dev)
    torch.manual_seed(7)
    for _, tile in VARIANTS:                                   # warm-up: workspaces, code objects
        timed_sample(d, args.batch, tile)
    runs = {name: [] for name, _ in VARIANTS}
    for _ in range(args.runs):
        for name, tile in VARIANTS:
            runs[name].append(timed_sample(d, args.batch, tile))
    n, halo = d.n_scales, _lib.TILE_HALO
    res = {"tool": "tile_ab", "config": args.config, "dim": args.dim, "batch": args.batch, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "CUs": torch.cuda.get_device_properties(0).multi_processor_count,
           "sizes_hw": [list(hw) for hw in d.image_sizes], "steps_per_scale": d.num_timesteps_ideal, "halo": halo}
    for name, rr in runs.items():
        per = [[r[s] for r in rr] for s in range(n)]
        tot = [sum(r) for r in rr]
        res[name] = {"scale_s_median": [round(statistics.median(p), 4) for p in per],
                     "scale_s_min_max": [[round(min(p), 4), round(max(p), 4)] for p in per],
                     "total_s_runs": [round(t, 4) for t in tot], "total_s_median": round(statistics.median(tot), 4)}
    for name, tile in VARIANTS[1:]:
        hy, hx = (halo if tile[0] else 0), (halo if tile[1] else 0)
        res[name]["area_ratio"] = [round((h + 2 * hy) * (w + 2 * hx) / (h * w), 3) for h, w in d.image_sizes]
        res[name]["time_ratio"] = [round(a / b, 3) for a, b in zip(res[name]["scale_s_median"], res["off"]["scale_s_median"])]
        res[name]["time_ratio_total"] = round(res[name]["total_s_median"] / res["off"]["total_s_median"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
