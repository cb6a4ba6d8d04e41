"""Cost of known-region conditioning (`keep_maps`: inpainting / outpainting) in the sampler chain.

    python tools/keep_ab.py [--config C2] [--dim 160] [--batch 16] [--runs 3] [--plain-only] [--tree DIR] [--out FILE.json]

Times whole-pyramid samples, per scale, of two variants in ONE process, interleaved after a warm-up sample of each:
  plain    `keep_maps = None`: the chain launches the <KEEP = false> tail kernels, the ones it launched before the option existed
  inpaint  `keep_maps` set at every scale (a synthetic known image, a mask with a centred hole of a third of each side,
           `functions.keep_mask_pyramid`): the <KEEP = true> tails read 16 B/px more (mask + 3 channels of the known image)
Times are host clocks around device-synchronised scale calls (MultiScaleGaussianDiffusion.sample / sample_via_scale: upsample +
re-noise + every reverse step of the scale).

`--plain-only --tree DIR` measures the plain variant alone with the package of another checkout (its own library beside its own
sources) -- a commit from before the option: alternate such runs with runs of this tree on one box to see whether the plain path
moved.  Prints one JSON line."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch


def timed_sample(d, batch):
    """One sample over the full pyramid; returns seconds per scale."""
    per_scale, img = [], None
    for s in range(d.n_scales):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = d.sample(batch_size=batch, s=0) if s == 0 else d.sample_via_scale(batch, img, s=s)
        torch.cuda.synchronize()
        per_scale.append(time.perf_counter() - t0)
        assert tuple(img.shape[2:]) == tuple(d.image_sizes[s]) and bool(torch.isfinite(img).all())
    return per_scale, img


def inpaint_maps(d, dev):
    from sinddm_amd.functions import keep_mask_pyramid
    from sinddm_amd.synth import hash_randn
    H, W = d.image_sizes[-1]
    full = torch.ones(H, W)
    full[H // 3:H - H // 3, W // 3:W - W // 3] = 0
    masks = keep_mask_pyramid(full, list(d.image_sizes))
    return {s: (masks[s].to(dev).contiguous(), (hash_randn((3,) + tuple(hw), 300 + s) * 0.6).clamp(-1, 1).to(dev))
            for s, hw in enumerate(d.image_sizes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dim", type=int, default=160)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("keep_ab.py measures on the GPU: no device found")
    import sinddm_amd
    from sinddm_amd.configs import build_diffusion
    dev = torch.device("cuda:0")
    net, d = build_diffusion(args.config, args.dim, dev)
    variants = {"plain": None}
    if not args.plain_only:
        variants["inpaint"] = inpaint_maps(d, dev)
    torch.manual_seed(7)

    def run(name):
        # (plain sets nothing: a `--tree` from before `sampling()` runs it)
        with d.sampling(keep_maps=variants[name]) if variants[name] is not None else contextlib.nullcontext():
            per, img = timed_sample(d, args.batch)
        if variants[name] is not None:                         # the kept pixels of the finest scale are the known image
            m, k0 = variants[name][d.n_scales - 1]
            assert torch.equal(img[:, :, m == 1], k0[None].expand_as(img)[:, :, m == 1])
        return per

    for name in variants:                                      # warm-up: workspaces, code objects
        run(name)
    runs = {name: [] for name in variants}
    for _ in range(args.runs):
        for name in variants:
            runs[name].append(run(name))
    res = {"tool": "keep_ab", "package": os.path.dirname(os.path.abspath(sinddm_amd.__file__)), "config": args.config,
           "dim": args.dim, "batch": args.batch, "runs": args.runs, "device": torch.cuda.get_device_name(0),
           "CUs": torch.cuda.get_device_properties(0).multi_processor_count,
           "sizes_hw": [list(hw) for hw in d.image_sizes], "steps_per_scale": d.num_timesteps_ideal}
    for name, rr in runs.items():
        per = [[r[s] for r in rr] for s in range(d.n_scales)]
        tot = [sum(r) for r in rr]
        res[name] = {"scale_s_median": [round(statistics.median(p), 4) for p in per],
                     "scale_s_min_max": [[round(min(p), 4), round(max(p), 4)] for p in per],
                     "total_s_runs": [round(t, 4) for t in tot], "total_s_median": round(statistics.median(tot), 4)}
    if "inpaint" in res:
        res["inpaint"]["time_ratio"] = [round(a / b, 4) for a, b in zip(res["inpaint"]["scale_s_median"], res["plain"]["scale_s_median"])]
        res["inpaint"]["time_ratio_total"] = round(res["inpaint"]["total_s_median"] / res["plain"]["total_s_median"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
