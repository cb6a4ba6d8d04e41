"""Cost of per-sample conditioning maps in the sampler chain: the time of one network evaluation + step tail of a keep run.

    python tools/batch_maps_time.py [--config C2] [--dim 160] [--batch 16] [--scale 1] [--steps 24] [--runs 3]
                                    [--variant shared|per_sample] [--tree DIR] [--out FILE.json]

One process times ONE variant of `_run_steps` at one scale with `keep_maps` set (a mask with a centred hole, a synthetic known
image): `shared` hands the chain one mask and one known image for the batch, `per_sample` B different ones (16 B/px more map
traffic per sample; sinddm_sample_chain_batch).  One warm-up run, then `--runs` timed runs of `--steps` reverse steps each
(t = steps - 1 ... 0); host clock around a device-synchronised call, divided by the number of steps.
`--tree DIR` takes the package of another checkout (its own library beside its own sources), e.g. the parent commit, which has
the shared variant only.  Alternate fresh processes of the variants on one box.  Prints one JSON line."""
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
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--variant", choices=("shared", "per_sample"), default="shared")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("batch_maps_time.py measures on the GPU: no device found")
    import sinddm_amd
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.synth import hash_randn
    dev = torch.device("cuda:0")
    net, d = build_diffusion(args.config, args.dim, dev)
    s, B = args.scale, args.batch
    H, W = d.image_sizes[s]
    m = torch.ones(H, W)
    m[H // 3:H - H // 3, W // 3:W - W // 3] = 0
    k0 = (hash_randn((3, H, W), 300 + s) * 0.6).clamp(-1, 1)
    if args.variant == "per_sample":                           # B different jobs: the hole and the known image move with b
        m = torch.stack([torch.roll(m, shifts=(b, 2 * b), dims=(0, 1)) for b in range(B)])
        k0 = torch.stack([(hash_randn((3, H, W), 400 + b) * 0.6).clamp(-1, 1) for b in range(B)])
    d.keep_maps = {s: (m.to(dev).contiguous(), k0.to(dev).contiguous())}
    x0 = (hash_randn((B, 3, H, W), 31 + s) * 0.8).to(dev)
    d.img_prev_upsample = (hash_randn((B, 3, H, W), 32 + s) * 0.5).clamp(-1, 1).to(dev)
    ts = list(range(args.steps - 1, -1, -1))
    torch.manual_seed(7)

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = d._run_steps(x0.clone(), s, ts)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        km, kx = d.keep_maps[s]
        known = (km == 1).expand(B, H, W)[:, None].expand(B, 3, H, W)
        assert bool(torch.isfinite(y).all()) and torch.equal(y[known], kx.expand(B, 3, H, W)[known])     # t = 0 ends the run
        return dt / len(ts)

    run()                                                      # warm-up: workspace, code objects
    per = [run() for _ in range(args.runs)]
    res = {"tool": "batch_maps_time", "package": os.path.dirname(os.path.abspath(sinddm_amd.__file__)), "variant": args.variant,
           "config": args.config, "dim": args.dim, "batch": B, "scale": s, "size_hw": [H, W], "steps": len(ts),
           "device": torch.cuda.get_device_name(0), "ms_per_eval_runs": [round(1e3 * v, 4) for v in per],
           "ms_per_eval_median": round(1e3 * statistics.median(per), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
