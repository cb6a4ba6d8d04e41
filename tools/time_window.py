"""Cost of a windowed known-region run (`keep_window`, sinddm_normal_fill_window) beside the full-image keep run.

    python tools/time_window.py --variant keep [--window N] [--config C2] [--dim 160] [--batch 16] [--scale 4] [--evals 24]
                                [--runs 5] [--out FILE.json]
    python tools/time_window.py --variant fill [--window 96] [--reps 200] ...
    python tools/time_window.py --all [--rounds 3] [--out FILE.jsonl]

One process times ONE variant at one scale of a config (C2 scale 4 is 186x248), synthetic closed-form weights, per-sample seeds:
    keep      `_run_steps` over the last `--evals` levels with a keep mask whose hole is a centred (N - 32) x (N - 32) square:
              `--window 0` runs the full image (`keep_window` off), `--window N` runs the N x N windows (margin 16).  ms per
              evaluation; for a windowed run also the ms per evaluation of its sinddm_normal_fill_window calls alone (the
              same pieces, the same ids), i.e. the fill's share.
    fill      one slot of sinddm_normal_fill_window at an N x N window against the trivial alternative: sinddm_normal_fill_samples
              of the whole 3 H W per sample plus the gather of the windows.  Microseconds per call over `--reps` calls between
              two device synchronisations.
One warm-up run, then `--runs` timed runs; host clock around a device-synchronised call.  Prints one JSON line.
`--all` does the alternating itself: fresh child processes, each under `--child_timeout` seconds, `--rounds` times the sequence
full, 64, 96, 128, then the fill comparison; one JSON line per child, appended to `--out`.  Compare the medians against the
spread of the repeated processes of one variant."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

WINDOWS = (0, 64, 96, 128)


def alternate(args):
    import subprocess
    me = os.path.abspath(__file__)
    common = ["--config", args.config, "--dim", str(args.dim), "--batch", str(args.batch), "--scale", str(args.scale),
              "--evals", str(args.evals), "--runs", str(args.runs)]
    plan = [("keep", n) for _ in range(args.rounds) for n in WINDOWS] + [("fill", 96)] * args.rounds
    for variant, n in plan:
        cmd = [sys.executable, me, "--variant", variant, "--window", str(n)] + common
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
        if r.returncode != 0:
            raise SystemExit(f"time_window.py: {' '.join(cmd)} ended with status {r.returncode}")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("keep", "fill"), default=None)
    ap.add_argument("--all", action="store_true", help="run the whole alternating comparison")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child_timeout", type=int, default=150)
    ap.add_argument("--window", type=int, default=96, metavar="N", help="0: the full image")
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dim", type=int, default=160)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--evals", type=int, default=24)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.all:
        return alternate(args)
    if args.variant is None:
        ap.error("--variant or --all is required")
    if args.variant == "fill" and args.window == 0:
        ap.error("--variant fill needs a window")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        raise SystemExit("time_window.py measures on the GPU: no device found")
    from sinddm_amd import _lib
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.models import _KeepWindow, noise_stream_id
    from sinddm_amd.sampler import RunPlan
    from sinddm_amd.synth import hash_randn
    dev = torch.device("cuda:0")
    s, B, n, N = args.scale, args.batch, args.evals, args.window
    net, d = build_diffusion(args.config, args.dim, dev)
    H, W = d.image_sizes[s]
    side = (N if N else 96) - 32
    if not 0 < side <= min(H, W) - 32:
        raise SystemExit(f"--window {N}: 64 ... {min(H, W)} (the hole is the window minus the margin of 16 on every side)")
    m = torch.ones(H, W, device=dev)
    y0, x0 = (H - side) // 2, (W - side) // 2
    m[y0:y0 + side, x0:x0 + side] = 0
    keep = {s: (m, (hash_randn((3, H, W), 40) * 0.6).clamp(-1, 1).to(dev))}
    d.img_prev_upsample = (hash_randn((B, 3, H, W), 42 + s) * 0.4).clamp(-1, 1).to(dev) if s > 0 else None
    x = (hash_randn((B, 3, H, W), 43 + s) * 0.8).to(dev)
    levels = list(range(n - 1, -1, -1))
    res = {"tool": "time_window", "device": torch.cuda.get_device_name(0), "variant": args.variant, "config": args.config,
           "dim": args.dim, "batch": B, "scale": s, "size_hw": [int(H), int(W)], "window": N}

    def timed(fn, per):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / per

    with d.sampling(keep_maps=keep, sample_seeds=[1000 + b for b in range(B)], keep_window=16 if N else None):
        if args.variant == "keep":
            plan = RunPlan(d, x, s, levels)
            assert (plan.window is None) == (N == 0) and (N == 0 or plan.window[:2] == (N, N)), plan.window
            run = lambda: d._run_steps(x.clone(), s, levels)
            assert bool(torch.isfinite(run()).all())               # warm-up: workspace, code objects
            per = [timed(run, n) for _ in range(args.runs)]
            res.update(evals=n, ms_per_eval_runs=[round(1e3 * v, 4) for v in per], ms_per_eval_median=round(1e3 * statistics.median(per), 4))
            if N:
                win = _KeepWindow(d, plan, x)
                ids = [noise_stream_id(s, "step", i) for i in range(n)]
                win.fill(ids)
                fill = [timed(lambda: win.fill(ids), n) for _ in range(args.runs)]
                res.update(fill_ms_per_eval_median=round(1e3 * statistics.median(fill), 4),
                           fill_share=round(statistics.median(fill) / statistics.median(per), 4))
        else:
            lib, reps = _lib.load(), args.reps
            plan = RunPlan(d, x, s, levels)
            win = _KeepWindow(d, plan, x)
            sid = noise_stream_id(s, "step", 0)
            seeds = torch.tensor(d.sample_seeds, dtype=torch.int64, device=dev)
            full = torch.empty((B, 3, H, W), device=dev)
            ids, out = torch.tensor([sid], dtype=torch.int64, device=dev), torch.empty((1, B, 3, N, N), device=dev)
            st = _lib.stream_ptr(dev)

            def window_fill():
                for _ in range(reps):
                    _lib.check(lib.sinddm_normal_fill_window(_lib.ptr(out), 1, _lib.ptr(ids), B, H, W, _lib.ptr(win.org), N, N,
                                                             _lib.ptr(win.kd), None, 1, st), "sinddm_normal_fill_window")

            def full_fill_and_slice():
                for _ in range(reps):
                    _lib.check(lib.sinddm_normal_fill_samples(_lib.ptr(full), B, 3 * H * W, _lib.ptr(seeds), sid, st),
                               "sinddm_normal_fill_samples")
                    win.crop(full)

            window_fill(), full_fill_and_slice()
            assert torch.equal(out[0], win.crop(full))             # (the two routes make the same numbers)
            a = [timed(window_fill, reps) for _ in range(args.runs)]
            b = [timed(full_fill_and_slice, reps) for _ in range(args.runs)]
            res.update(reps=reps, window_fill_us=round(1e6 * statistics.median(a), 2),
                       full_fill_and_slice_us=round(1e6 * statistics.median(b), 2),
                       window_fill_us_runs=[round(1e6 * v, 2) for v in a], full_fill_and_slice_us_runs=[round(1e6 * v, 2) for v in b])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
