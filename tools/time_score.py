"""Cost of a denoising-score evaluation (sinddm_score_chain) beside a sampler step and beside the route a user had before.

    python tools/time_score.py --variant {score,chain,composed} [--config C2] [--dim 160] [--batch 16] [--scale 1]
                               [--evals 48] [--runs 5] [--tree DIR] [--out FILE.json]
    python tools/time_score.py --ab PARENT_DIR [--rounds 3] [--scale 1] [--evals 48] [--runs 5] [--out FILE.jsonl]

One process times ONE variant at one scale of a config (C2 scale 1 is 67x90, scale 4 is 186x248), synthetic closed-form weights:
    score     `MultiScaleGaussianDiffusion.denoise_score` with `--evals` levels, one draw, per-sample seeds: one
              sinddm_score_chain call -- per evaluation the network's launches, whose last one scores and draws the next x_t
    chain     `_run_steps` over `--evals` reverse steps: one sinddm_sample_chain call, ms per evaluation + tail of the plain
              sampler (one stream: `two_streams` off, as the score call has no second stream; `--two_streams` turns it on)
    composed  what a user would write without the score call: per evaluation torch.randn_like, sinddm_q_sample, the TRAINING
              forward (`denoise_fn(x, t, s)` in grad mode: the activation-saving forward p_losses runs), torch abs / sum
One warm-up run, then `--runs` timed runs; host clock around a device-synchronised call, divided by the number of evaluations.
`--tree DIR` takes the package of another checkout (its own library beside its own sources), e.g. the parent commit, which has
the `chain` and `composed` variants only.  Prints one JSON line.
`--ab PARENT_DIR` does the alternating itself: fresh child processes, each under `--child_timeout` seconds, the parent's `chain`
and this tree's `score` `--rounds` times in turn, then this tree's `chain` and the `composed` route of both trees; one JSON line
per child, appended to `--out`.  Compare the medians against the spread of the repeated processes of one variant."""
import argparse
import json
import os
import statistics
import sys
import time

import torch


def alternate(args):
    """--ab PARENT: the whole comparison at one scale, every measurement a fresh child process under its own time limit, the
    parent's chain and this tree's score chain alternating `--rounds` times, then this tree's chain and the composed route of
    both trees.  The children's JSON lines go to stdout and, appended, to `--out`.  Stops at the first child that fails."""
    import subprocess
    me = os.path.abspath(__file__)
    common = ["--config", args.config, "--dim", str(args.dim), "--batch", str(args.batch), "--scale", str(args.scale),
              "--evals", str(args.evals), "--runs", str(args.runs)] + (["--two_streams"] if args.two_streams else [])
    plan = []
    for _ in range(args.rounds):
        plan += [("chain", args.ab), ("score", None)]
    plan += [("chain", None), ("composed", None), ("composed", args.ab)]
    for variant, tree in plan:
        cmd = [sys.executable, me, "--variant", variant] + common + (["--tree", tree] if tree else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
        if r.returncode != 0:
            raise SystemExit(f"time_score.py: {' '.join(cmd)} ended with status {r.returncode}")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("score", "chain", "composed"), default=None)
    ap.add_argument("--ab", default=None, metavar="PARENT", help="run the whole alternating comparison against this checkout")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child_timeout", type=int, default=150)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dim", type=int, default=160)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--evals", type=int, default=48)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--two_streams", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.ab is not None:
        return alternate(args)
    if args.variant is None:
        ap.error("--variant or --ab is required")
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("time_score.py measures on the GPU: no device found")
    import sinddm_amd
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.synth import hash_randn
    dev = torch.device("cuda:0")
    s, B, n = args.scale, args.batch, args.evals
    net, d = build_diffusion(args.config, args.dim, dev)
    H, W = d.image_sizes[s]
    T = d.num_timesteps_trained[s]
    if not 1 <= n <= T:
        raise SystemExit(f"--evals {n} outside 1 ... {T}")
    y = (hash_randn((B, 3, H, W), 41 + s) * 0.5).clamp(-1, 1).to(dev)
    yp = (hash_randn((B, 3, H, W), 42 + s) * 0.4).clamp(-1, 1).to(dev) if s > 0 else None
    levels = list(range(n - 1, -1, -1))                        # the sampler's last n levels: one arithmetic run in every variant
    torch.manual_seed(7)

    if args.variant == "score":
        seeds = [1000 + b for b in range(B)]

        def once():
            smap, table = d.denoise_score(y, s, y_prev=yp, levels=levels, draws=1, seeds=seeds)
            return smap
    elif args.variant == "chain":
        d.two_streams = bool(args.two_streams)
        d.img_prev_upsample = yp
        x0 = (hash_randn((B, 3, H, W), 43 + s) * 0.8).to(dev)

        def once():
            return d._run_steps(x0.clone(), s, levels)
    else:
        gamma_row = d.gammas[s - 1].contiguous() if s > 0 else None

        def once():
            smap = torch.zeros(B, H, W, device=dev)
            for t in levels:                                   # (grad mode on: the forward p_losses runs, activations saved)
                z = torch.randn_like(y)
                tt = torch.full((B,), t, device=dev, dtype=torch.long)
                x_t = d._q_sample_impl(yp if s > 0 else y, tt, 0, z, x_orig=y if s > 0 else None, gamma_row=gamma_row)
                eps = d.denoise_fn(x_t, tt, s).detach()
                smap += (z - eps).abs().sum(dim=1)
            return smap

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = once()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(out).all())
        return dt / n

    run()                                                      # warm-up: workspace, code objects
    per = [run() for _ in range(args.runs)]
    res = {"tool": "time_score", "package": os.path.relpath(os.path.dirname(os.path.abspath(sinddm_amd.__file__))),
           "device": torch.cuda.get_device_name(0), "variant": args.variant, "two_streams": bool(args.two_streams),
           "config": args.config, "dim": args.dim, "batch": B, "scale": s, "size_hw": [int(H), int(W)], "evals": n,
           "ms_per_eval_runs": [round(1e3 * v, 4) for v in per], "ms_per_eval_median": round(1e3 * statistics.median(per), 4),
           "ms_per_eval_min": round(1e3 * min(per), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
