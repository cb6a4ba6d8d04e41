"""Cost of seed blending (`seed_mix`) in the sampler chain.

    python tools/mix_ab.py [--config C2] [--dim 160] [--batch 16] [--scales 0 1 4] [--steps 60] [--runs 3]
                           [--plain-only] [--tree DIR] [--out FILE.json]

Times runs of `--steps` reverse steps (the last ones of the scale, ending at t = 0) of the named scales -- C2: scale 0 = 48x64
(plain fused tail, real sigma), scale 1 = 67x90 (padded-row tail, two streams), scale 4 = the finest, 186x248 (plain fused
tail) -- of these variants in ONE process, interleaved after a warm-up run of each:
  plain     no seeds: one 62-bit seed for the run, the whole-batch noise index
  seeded    `sample_seeds`: sinddm_sample_chain_seeds, the tails load their sample's key
  mix1/2/3  `seed_mix` with K = 1, 2, 3 seeds per sample: sinddm_sample_chain_mix, K Philox + Box-Muller draws per quad
  recorded  `noise_fn` + `chain_noise` handing over a buffer that is already on the device: the tails read 12 B/px of draws
            (the host's cost of COMPOSING that buffer -- K fills per step -- is not in the figure)
Times are host clocks around device-synchronised `_run_steps` calls, so they include uploading the tables.

`--plain-only --tree DIR` measures the plain variant alone with the package of another checkout (its own library beside its own
sources) -- a commit from before the option: alternate such runs with runs of this tree on one box to see whether the plain path
moved.  Prints one JSON line."""
import argparse
import contextlib
import json
import math
import os
import statistics
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dim", type=int, default=160)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--scales", type=int, nargs="+", default=[0, 1, 4])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("mix_ab.py measures on the GPU: no device found")
    import sinddm_amd
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.synth import hash_randn
    dev = torch.device("cuda:0")
    net, d = build_diffusion(args.config, args.dim, dev)
    variants = ["plain"] if args.plain_only else ["plain", "seeded", "mix1", "mix2", "mix3", "recorded"]
    B = args.batch
    seeds = [1000 + b for b in range(B)]

    def mix(K):                                               # K seeds per sample, every weight at work
        return [[1000 + b + 100 * k for k in range(K)] for b in range(B)], [[1.0 / math.sqrt(K)] * K for _ in range(B)]

    torch.manual_seed(7)
    res = {"tool": "mix_ab", "package": os.path.dirname(os.path.abspath(sinddm_amd.__file__)), "config": args.config,
           "dim": args.dim, "batch": B, "steps": args.steps, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "CUs": torch.cuda.get_device_properties(0).multi_processor_count,
           "scales": {}}
    for s in args.scales:
        H, W = d.image_sizes[s]
        x0 = (hash_randn((B, 3, H, W), 31 + s) * 0.8).to(dev)
        d.img_prev_upsample = (hash_randn((B, 3, H, W), 32 + s) * 0.5).clamp(-1, 1).to(dev)
        ts = list(reversed(range(args.steps)))
        rec_z = torch.randn((B, 3, H, W), device=dev) if "recorded" in variants else None

        def run(name):
            opts = {}
            if name == "seeded":
                opts = dict(sample_seeds=seeds)
            elif name.startswith("mix"):
                opts = dict(seed_mix=mix(int(name[3:])))
            elif name == "recorded":
                opts = dict(noise_fn=lambda kind, shape, ss, tt, dv: rec_z, chain_noise=True)
            with d.sampling(**opts) if opts else contextlib.nullcontext():     # (plain: a `--tree` from before `sampling()`)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                y = d._run_steps(x0, s, ts)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            assert bool(torch.isfinite(y).all())
            return dt / args.steps * 1e3

        for name in variants:                                  # warm-up: workspaces, code objects
            run(name)
        ms = {name: [] for name in variants}
        for _ in range(args.runs):
            for name in variants:
                ms[name].append(run(name))
        rec = {"hw": [H, W]}
        for name in variants:
            rec[name] = {"ms_per_step_runs": [round(v, 4) for v in ms[name]],
                         "ms_per_step_median": round(statistics.median(ms[name]), 4),
                         "ms_per_step_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)]}
        for name in variants[2:]:
            rec[name + "_over_seeded"] = round(rec[name]["ms_per_step_median"] / rec["seeded"]["ms_per_step_median"], 4)
        res["scales"][str(s)] = rec
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
