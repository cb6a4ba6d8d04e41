"""Cost of layout conditioning (`layout_maps`, sinddm_sample_chain_layout) on one scale of the sampler chain.

    python tools/layout_time.py --scale 1 --mode plain|all|half [--config C2] [--dim 160] [--batch 16] [--down 8] [--runs 3]

ONE configuration per process (alternate fresh processes of the configurations on one box): `_run_steps` of one whole scale --
every reverse step of `p_sample_via_scale_loop` -- at the given batch with in-kernel noise, one warm-up run and `--runs` timed
runs, host clocks around device-synchronised calls.
  plain   no layout: the fused chain as it always ran
  all     every step conditioned (t_min = 0): the worst case, every step unfused + the block-delta kernel
  half    t_min at half the run: the upper half of the steps conditioned
Prints one JSON line."""
import argparse
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
    ap.add_argument("--scale", type=int, required=True)
    ap.add_argument("--mode", choices=("plain", "all", "half"), required=True)
    ap.add_argument("--down", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        raise SystemExit("layout_time.py measures on the GPU: no device found")
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.synth import hash_randn
    dev = torch.device("cuda:0")
    net, d = build_diffusion(args.config, args.dim, dev)
    s = args.scale
    H, W = d.image_sizes[s]
    n = d.num_timesteps_ideal[s] - 1 if s > 0 else d.num_timesteps
    t_seq = list(reversed(range(0, n)))
    x0 = (hash_randn((args.batch, 3, H, W), 31 + s) * 0.8).to(dev)
    d.img_prev_upsample = (hash_randn((args.batch, 3, H, W), 32 + s) * 0.5).clamp(-1, 1).to(dev)
    t_min = {"plain": None, "all": 0, "half": n // 2}[args.mode]
    opts = {}
    if t_min is not None:
        opts = dict(layout_maps={s: (hash_randn((3, H, W), 83) * 0.6).clamp(-1, 1).to(dev)}, layout_down={s: args.down},
                    layout_strength=1.0, layout_t_min=t_min)
    torch.manual_seed(7)

    def run():
        with d.sampling(**opts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = d._run_steps(x0, s, t_seq)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        assert bool(torch.isfinite(y).all())
        return dt

    run()
    times = [run() for _ in range(args.runs)]
    print(json.dumps({"tool": "layout_time", "config": args.config, "dim": args.dim, "batch": args.batch, "scale": s,
                      "size_hw": [H, W], "mode": args.mode, "down": args.down, "evaluations": n,
                      "conditioned": 0 if t_min is None else sum(1 for t in t_seq if t >= t_min),
                      "ms_runs": [round(1e3 * t, 2) for t in times],
                      "ms_per_eval_median": round(1e3 * statistics.median(times) / n, 4),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
