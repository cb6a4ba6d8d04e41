"""A/B of ROI-guided sampling: one fused chain call per scale (`chain_guided = True`, sinddm_sample_chain_ex with edit maps)
against the step-by-step route (`chain_guided = False`: per step sinddm_net_forward + torch.randn + sinddm_reverse_step_edit).

    python tools/roi_chain_ab.py [--config C2] [--dim 160] [--batch 16] [--runs 3] [--out FILE.json]
    python tools/roi_chain_ab.py --once chain|stepwise        # warm-up + ONE run of one variant (for a kernel trace)

Same process, same library, closed-form weights, a synthetic pyramid of the configuration's sizes; one warm-up run of each
variant, then `--runs` timed runs of each, interleaved.  Times are host clocks around device-synchronised scale calls
(MultiScaleGaussianDiffusion.sample / sample_via_scale, i.e. upsample + re-noise + every reverse step of the scale).  The
finest scale is never guided: it is the control.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_trainer(cfg_name, dim, dev, tmp):
    from PIL import Image
    from sinddm_amd.configs import CONFIGS, build_diffusion
    from sinddm_amd.trainer import MultiscaleTrainer
    cfg = CONFIGS[cfg_name]
    n = len(cfg["sizes"])
    rng = np.random.RandomState(1234)
    for i, (w, h) in enumerate(cfg["sizes"]):
        for sub in (f"scale_{i}", f"scale_{i}_recon"):
            os.makedirs(os.path.join(tmp, sub), exist_ok=True)
            Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(tmp, sub, "synthetic.png"))
    net, d = build_diffusion(cfg_name, dim, dev)
    tr = MultiscaleTrainer(d, folder=tmp + "/", n_scales=n, scale_factor=cfg["scale_factor"], image_sizes=cfg["sizes"],
                           train_batch_size=1, train_lr=1e-3, train_num_steps=1, gradient_accumulate_every=1,
                           step_start_ema=10 ** 9, update_ema_every=10, save_and_sample_every=10 ** 9, avg_window=2,
                           results_folder=os.path.join(tmp, "results"), device=dev)
    return tr, cfg


def timed_run(tr, batch, boxes, target, chain_guided):
    """One roi_guided_sampling over the full pyramid; returns seconds per scale."""
    em = tr.ema_model
    em.chain_guided = chain_guided
    per_scale = []
    sample, via = em.sample, em.sample_via_scale

    def wrap(fn):
        def run(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            per_scale.append(time.perf_counter() - t0)
            return out
        return run

    em.sample, em.sample_via_scale = wrap(sample), wrap(via)
    try:
        outs = tr.roi_guided_sampling(target_roi=target, roi_bb_list=boxes, save_unbatched=False, batch_size=batch,
                                      scale_mul=(1, 1), save_images=False)
    finally:
        del em.sample, em.sample_via_scale                     # (instance attributes shadowing the methods)
        em.chain_guided = True
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    return per_scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dim", type=int, default=160)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--once", choices=["chain", "stepwise"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roi_chain_ab.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="sinddm_roi_ab_")
    try:
        tr, cfg = make_trainer(args.config, args.dim, dev, tmp)
        W, H = cfg["sizes"][-1]
        # two overlapping boxes [y, x, h, w] and the patch they are pulled towards, as fractions of the full image
        boxes = [[int(.22 * H), int(.24 * W), int(.43 * H), int(.29 * W)], [int(.38 * H), int(.40 * W), int(.32 * H), int(.24 * W)]]
        target = [int(.11 * H), int(.10 * W), int(.32 * H), int(.32 * W)]
        torch.manual_seed(7)
        if args.once:
            guided = args.once == "chain"
            timed_run(tr, args.batch, boxes, target, guided)
            t = timed_run(tr, args.batch, boxes, target, guided)
            print(json.dumps({"variant": args.once, "seconds_per_scale": [round(v, 4) for v in t], "total_s": round(sum(t), 4)}))
            return
        for v in (False, True):                               # warm-up: workspaces, code objects, edit maps
            timed_run(tr, args.batch, boxes, target, v)
        runs = {"stepwise": [], "chain": []}
        for _ in range(args.runs):
            for name, v in (("stepwise", False), ("chain", True)):
                runs[name].append(timed_run(tr, args.batch, boxes, target, v))
        n = len(cfg["sizes"])
        res = {"tool": "roi_chain_ab", "config": args.config, "dim": args.dim, "batch": args.batch, "runs": args.runs,
               "device": torch.cuda.get_device_name(0), "CUs": torch.cuda.get_device_properties(0).multi_processor_count,
               "sizes_hw": [[h, w] for (w, h) in cfg["sizes"]], "steps_per_scale": tr.ema_model.num_timesteps_ideal,
               "guided_scales": list(range(n - 1))}
        for name, rr in runs.items():
            per = [[r[s] for r in rr] for s in range(n)]
            tot = [sum(r) for r in rr]
            res[name] = {"scale_s_median": [round(statistics.median(p), 4) for p in per],
                         "scale_s_min_max": [[round(min(p), 4), round(max(p), 4)] for p in per],
                         "total_s_runs": [round(t, 4) for t in tot], "total_s_median": round(statistics.median(tot), 4)}
        res["chain_over_stepwise_per_scale"] = [round(c / s, 4) for c, s in zip(res["chain"]["scale_s_median"],
                                                                                 res["stepwise"]["scale_s_median"])]
        res["chain_over_stepwise_total"] = round(res["chain"]["total_s_median"] / res["stepwise"]["total_s_median"], 4)
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
