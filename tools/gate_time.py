"""Cost of the level gate (`keep_gated`: per-pixel edit strength) in the sampler chain, and the bytes of the ungated keep run.

    python tools/gate_time.py [--config C2] [--dim 160] [--batch 16] [--scale 1] [--steps 24] [--runs 3]
                              [--variant ungated|gated] [--tree DIR] [--out FILE.json]
    python tools/gate_time.py --digest [--tree DIR] [--out FILE.json]

Timing: one process times ONE variant of `_run_steps` at one scale with `keep_maps` set (a hold map with plateaus at 0, 0.25,
0.5, 0.6 and 1, a synthetic known image): `ungated` reads the map as the blend weight it has always been, `gated` sets
`keep_gated` (sinddm_sample_chain_gate: the same kernels with a threshold per step).  One warm-up run, then `--runs` timed runs of
`--steps` reverse steps each (t = steps - 1 ... 0); host clock around a device-synchronised call, divided by the number of
steps: ms per network evaluation + tail.  C2 scale 1 is 67x90, scale 4 is 186x248.
`--tree DIR` takes the package of another checkout (its own library beside its own sources, with `sampling()`), e.g. the parent
commit.  Alternate fresh processes of the variants on one box.
`--digest`: the SHA-256 of the result of an ungated keep run of `_run_steps` on the four shapes of the tail kernels (plain fused,
padded rows with two streams, padded rows, unfused; three steps incl. t = 0; torch.manual_seed fixed) -- run it with this tree
and with `--tree` of the parent and compare: the option must not move a byte of the run without it.  Prints one JSON line."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import torch

SHAPES = [("C2", 160, 0, 16, False, [700, 2, 0]), ("C2", 160, 1, 16, True, [400, 1, 0]), ("C2", 160, 3, 4, False, [311, 2, 0]),
          ("C2", 20, 3, 4, False, [311, 2, 0])]


def hold_map(H, W):
    h = torch.zeros(H, W)
    h[5:25, 8:32] = 1
    h[14:31, 13:43] = 0.25
    h[3:13, 33:47] = 0.5
    h[27:41, 5:19] = 0.6
    h[H - 11:, W - 9:] = 1
    return h


def setup(config, dim, s, B, dev):
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.synth import hash_randn
    net, d = build_diffusion(config, dim, dev)
    H, W = d.image_sizes[s]
    k0 = (hash_randn((3, H, W), 300 + s) * 0.6).clamp(-1, 1)
    maps = {s: (hold_map(H, W).to(dev).contiguous(), k0.to(dev).contiguous())}
    x0 = (hash_randn((B, 3, H, W), 31 + s) * 0.8).to(dev)
    d.img_prev_upsample = (hash_randn((B, 3, H, W), 32 + s) * 0.5).clamp(-1, 1).to(dev)
    return d, maps, x0, (H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dim", type=int, default=160)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--variant", choices=("ungated", "gated"), default="ungated")
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("gate_time.py measures on the GPU: no device found")
    import sinddm_amd
    dev = torch.device("cuda:0")
    res = {"tool": "gate_time", "package": os.path.dirname(os.path.abspath(sinddm_amd.__file__)),
           "device": torch.cuda.get_device_name(0)}
    if args.digest:
        res["digest"] = {}
        for cfg, dim, s, B, aux, ts in SHAPES:
            d, maps, x0, (H, W) = setup(cfg, dim, s, B, dev)
            torch.manual_seed(1234 + s)
            with d.sampling(keep_maps=maps, two_streams=aux):
                y = d._run_steps(x0.clone(), s, ts)
                torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all())
            res["digest"][f"{cfg}_dim{dim}_s{s}_{H}x{W}_B{B}"] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
    else:
        s, B = args.scale, args.batch
        d, maps, x0, (H, W) = setup(args.config, args.dim, s, B, dev)
        ts = list(range(args.steps - 1, -1, -1))
        torch.manual_seed(7)

        def run():
            with d.sampling(keep_maps=maps, keep_gated=args.variant == "gated"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                y = d._run_steps(x0.clone(), s, ts)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            km, kx = maps[s]
            known = (km == 1).expand(B, H, W)[:, None].expand(B, 3, H, W)
            assert bool(torch.isfinite(y).all()) and torch.equal(y[known], kx.expand(B, 3, H, W)[known])     # t = 0 ends the run
            return dt / len(ts)

        run()                                                  # warm-up: workspace, code objects
        per = [run() for _ in range(args.runs)]
        res.update({"variant": args.variant, "config": args.config, "dim": args.dim, "batch": B, "scale": s, "size_hw": [H, W],
                    "steps": len(ts), "ms_per_eval_runs": [round(1e3 * v, 4) for v in per],
                    "ms_per_eval_median": round(1e3 * statistics.median(per), 4)})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
