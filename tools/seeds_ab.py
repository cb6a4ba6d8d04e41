"""Cost of per-sample noise seeds (`sample_seeds`) in the sampler chain.

    python tools/seeds_ab.py [--config C2] [--dim 160] [--batch 16] [--scales 1 4] [--steps 60] [--runs 5]
                             [--plain-only] [--tree DIR] [--out FILE.json]

Times runs of `--steps` reverse steps (the last ones of the scale, ending at t = 0) of the named scales -- C2: scale 1 = 67x90
(padded-row tail, two streams), scale 4 = the finest, 186x248 (plain fused tail) -- of two variants in ONE process,
interleaved after a warm-up run of each:
  plain   `sample_seeds = None`: sinddm_sample_chain_ex, one 62-bit seed for the run, the whole-batch noise index
  seeded  `sample_seeds` set: sinddm_sample_chain_seeds, the tails load their sample's key (one scalar 8-byte load per block)
Times are host clocks around device-synchronised `_run_steps` calls, so the seeded figure includes uploading the seed array.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dim", type=int, default=160)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("seeds_ab.py measures on the GPU: no device found")
    import sinddm_amd
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.synth import hash_randn
    dev = torch.device("cuda:0")
    net, d = build_diffusion(args.config, args.dim, dev)
    variants = ["plain"] if args.plain_only else ["plain", "seeded"]
    seeds = [1000 + b for b in range(args.batch)]
    torch.manual_seed(7)
    res = {"tool": "seeds_ab", "package": os.path.dirname(os.path.abspath(sinddm_amd.__file__)), "config": args.config,
           "dim": args.dim, "batch": args.batch, "steps": args.steps, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "CUs": torch.cuda.get_device_properties(0).multi_processor_count,
           "scales": {}}
    for s in args.scales:
        H, W = d.image_sizes[s]
        x0 = (hash_randn((args.batch, 3, H, W), 31 + s) * 0.8).to(dev)
        d.img_prev_upsample = (hash_randn((args.batch, 3, H, W), 32 + s) * 0.5).clamp(-1, 1).to(dev)
        ts = list(reversed(range(args.steps)))

        def run(name):
            # (plain sets nothing: a `--tree` from before `sampling()` runs it)
            with d.sampling(sample_seeds=seeds) if name == "seeded" else contextlib.nullcontext():
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
        if "seeded" in rec:
            rec["seeded_over_plain"] = round(rec["seeded"]["ms_per_step_median"] / rec["plain"]["ms_per_step_median"], 4)
        res["scales"][str(s)] = rec
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
