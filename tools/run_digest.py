"""SHA-256 digests of what the sampler's PYTHON routes compute, to compare two checkouts bit for bit.

    python tools/run_digest.py [--tree DIR] [--out FILE.txt]

Where tools/chain_digest.py drives the C ABI, this drives `MultiScaleGaussianDiffusion`: `--tree DIR` imports the package of
another checkout (its own library beside its own sources).  Run it on two trees on ONE box, each in a fresh process, and
`diff` the outputs: a change of the host side that is meant to leave the numbers alone must leave every line alone.  Each
line is the digest of a result followed by the digest of the run's `draw_log` (tuples by repr, tensors as bytes).

Runs, C2 at dim 20, B = 3, omega = 0.3: scale 1 on 8x12 (fused tail) and 5x7 (unfused tail), steps [5 .. 0]; scale 0 on 8x12 from
T - 1 (mode 0).  For every option of OPTIONS (each sampler option alone and the pairs that are built):
  * `_run_steps` on the chain route with each noise source: torch's seed, `sample_seeds`, `seed_mix` (K = 2), and `noise_fn` with
    `chain_noise` under a CHAIN_NOISE_BYTES of two steps, so that the run is cut into three pieces;
  * the same run forced onto the step-by-step route: `noise_fn` without `chain_noise`, and -- under ROI guidance --
    `chain_guided = False` with the three other sources;
  * a bare `_p_sample_host_t` loop over the same walk (schedules from functions.py, `_solver_q`).
Then C2 dim 160 scale 1 at B = 16 with `two_streams` on and off (the aux stream is passed from Python), and one full pyramid
of C1 at dim 20 through `sample` / `sample_via_scale`.
Then the `drivers` section: `MultiscaleTrainer` on the C1 recipe of the GPU tests (the pyramid of tests/golden/c1_pyramid.npz,
closed-form weights, dim 32, T = 20), batch 2, seeds [11, 77]: `sample_scales` with `seeds` and with a K = 2 `seed_mix`,
`inpaint` with `window=None` and `window=16`, `outpaint((1, 1.5))`, `edit` with a ramp strength, `paint2image`, and
`roi_guided_sampling` shared and `per_sample`; one line per scale batch plus the `draw_log` digest each.
The digests depend on the kernels too: for A/B runs, not a fixture."""
import argparse
import contextlib
import hashlib
import json
import math
import os
import sys
import tempfile

import torch

B, STEPS = 3, [5, 4, 3, 2, 1, 0]
SEEDS, MIX = [11, 2 ** 40 + 5, 77], ([[3, 4], [5, 6], [7, 8]], [[1.0, 0.0], [0.6, 0.8], [math.sqrt(0.5), math.sqrt(0.5)]])
OPTIONS = ["plain", "roi", "tile", "keep", "keep_b", "resample", "layout", "layout_gain", "steps4_t", "steps4_logsnr", "order2",
           "eta0", "roi+tile", "roi+keep_b", "roi+resample", "roi+layout_gain", "tile+keep", "tile+layout", "tile+order2",
           "keep+resample", "keep_b+layout_gain", "keep+order2", "steps4_t+order2", "steps4_logsnr+eta0", "roi+steps4_t"]


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p.detach().cpu().contiguous().numpy().tobytes() if isinstance(p, torch.Tensor) else repr(p).encode())
    return h.hexdigest()


def log_digest(log):
    return sha(*[v for e in (log or []) for v in e])


def c1_trainer(tmp, dev):
    """The trainer of the `drivers` section, its data folder and results under `tmp`."""
    import numpy as np
    from PIL import Image
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    from sinddm_amd.synth import closed_form_state_dict
    from sinddm_amd.trainer import MultiscaleTrainer
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    with open(os.path.join(golden, "g11_img_scales.json")) as f:
        meta = json.load(f)["C1"]
    pyr, folder, res = np.load(os.path.join(golden, "c1_pyramid.npz")), os.path.join(tmp, "balloons") + "/", os.path.join(tmp, "res")
    for key in pyr.files:
        os.makedirs(folder + key, exist_ok=True)
        Image.fromarray(pyr[key]).save(folder + key + "/balloons.png")
    net = SinDDMNet(dim=32, multiscale=True, device=dev).to(dev)
    net.load_state_dict(closed_form_state_dict(32))
    sizes = [tuple(s) for s in meta["sizes"]]
    d = MultiScaleGaussianDiffusion(net, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"], image_sizes=sizes,
                                    timesteps=20, train_full_t=True, scale_losses=meta["rescale_losses"], loss_factor=1,
                                    loss_type="l1", device=dev, reblurring=True, omega=0, results_folder=res).to(dev)
    return MultiscaleTrainer(d, folder=folder, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"], image_sizes=sizes,
                             train_batch_size=2, train_lr=1e-3, train_num_steps=6, gradient_accumulate_every=1, step_start_ema=2,
                             update_ema_every=2, save_and_sample_every=10 ** 9, avg_window=2, sched_milestones=[3],
                             results_folder=res, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("run_digest.py runs on the GPU: no device found")
    from sinddm_amd import _lib, models
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.functions import resample_schedule, stride_schedule
    from sinddm_amd.synth import hash_randn
    print("package:", os.path.dirname(os.path.abspath(models.__file__)), file=sys.stderr)
    lib, dev, lines = _lib.load(), torch.device("cuda:0"), []
    budget0 = models.CHAIN_NOISE_BYTES

    def emit(name, y, log=None):
        if not bool(torch.isfinite(y).all()):
            raise SystemExit(f"non-finite result: {name}")
        lines.append(f"{sha(y)} {log_digest(log)}  {name}")
        print(lines[-1], flush=True)

    def keyed_noise():
        """A `noise_fn` whose draw depends on (kind, t) and on how many draws came before it: the order is in the digest."""
        count = [0]

        def fn(kind, shape, s, t, device):
            count[0] += 1
            z = torch.empty(shape, device=device)
            _lib.check(lib.sinddm_normal_fill(_lib.ptr(z), z.numel(), 4242 + count[0], 2 * t + (kind == "jump"),
                                              _lib.stream_ptr(device)), "sinddm_normal_fill")
            return z
        return fn

    def rnd(shape, key, a=0.6):
        return (hash_randn(shape, key) * a).clamp(-1, 1).to(dev)

    def scope(d, **opts):
        """`d.sampling(**opts)`; the same by hand for a `--tree` from before the scope existed."""
        if hasattr(d, "sampling"):
            return d.sampling(**opts)
        stack = contextlib.ExitStack()
        for k, v in opts.items():
            stack.callback(setattr, d, k, getattr(d, k))
            setattr(d, k, v)
        return stack

    def options(d, opt, s, H, W, steps):
        """The sampling options `opt` names (the boxes and patches of "roi" are plain state: set on d, and left there)."""
        out = {}
        put = out.update
        for o in opt.split("+"):
            if o == "roi":
                f = d.scale_factor ** (d.n_scales - s - 1)
                put(roi_guided_sampling=True)
                d.roi_bbs = [[int(math.ceil(v * f + 1e-6)) for v in (1, 2, 3, 4)]]
                d.roi_target_patch = [rnd((1, 3, 4, 5), 90 + i) for i in range(d.n_scales)]
            elif o == "tile":
                put(tile=(False, True))
            elif o in ("keep", "keep_b"):
                lead = (B,) if o == "keep_b" else ()
                put(keep_maps={s: ((rnd(lead + (H, W), 5, 1.0) > 0).float(), rnd(lead + (3, H, W), 6))})
            elif o == "resample":
                put(resample=(2, 2))
            elif o in ("layout", "layout_gain"):
                put(layout_maps={s: rnd(((B,) if o == "layout_gain" else ()) + (3, H, W), 7)}, layout_down={s: 3},
                    layout_strength=0.75, layout_t_min=steps[-3], layout_gain=[0.5, 1.0, 0.25] if o == "layout_gain" else None)
            elif o in ("steps4_t", "steps4_logsnr"):
                put(sample_steps=4, sample_spacing=o[7:])
            elif o == "order2":
                put(solver_order=2)
            elif o == "eta0":
                put(eta=0.0)
        return out

    def run(d, name, img, s, steps, **attrs):
        """One `_run_steps` with `attrs` set for the call; the result and the draw log go to the digest."""
        torch.manual_seed(7)
        with scope(d, draw_log=[], **attrs):
            y = d._run_steps(img.clone(), s, steps)
            torch.cuda.synchronize()
            emit(name, y, d.draw_log)

    def bare_loop(d, name, img, s, steps):
        """The walk `_run_steps` would take, driven through `_p_sample_host_t` by hand."""
        lands = q = None
        few = d._few_step_cfg(s)
        if few is not None:
            steps, lands = stride_schedule(steps, few[0] if few[0] is not None else len(steps), few[1],
                                           d._kappa(s) if few[1] == "logsnr" else None)
            q = d._solver_q(s, steps, lands) if few[2] == 2 else None
        jumps = [None] * len(steps)
        if d._resample_cfg() is not None:
            steps, jumps = resample_schedule(steps, *d._resample_cfg())
        x, hist = img.clone(), torch.empty_like(img) if q is not None else None
        with scope(d, noise_fn=keyed_noise()):
            for i, t in enumerate(steps):
                x = d._p_sample_host_t(x, t, s, step_pos=i, jump_to=jumps[i], land=lands[i] if lands is not None else None,
                                       q=q[i] if q is not None else None, hist=hist)
            torch.cuda.synchronize()
            emit(name, x)

    net, d = build_diffusion("C2", dim=20, device=dev)
    d.omega = 0.3
    T = d.num_timesteps
    for s, H, W, steps in [(1, 8, 12, STEPS), (1, 5, 7, STEPS), (0, 8, 12, list(range(T - 1, T - 7, -1)))]:
        img = (hash_randn((B, 3, H, W), 31 + s) * 0.8).to(dev)
        d.img_prev_upsample = rnd((B, 3, H, W), 32 + s, 0.5)
        for opt in OPTIONS:
            if "roi" in opt and s >= d.n_scales - 1:
                continue
            with scope(d, **options(d, opt, s, H, W, steps)):
                tag = f"s{s} {H}x{W} {opt}"
                hx = _lib.TILE_HALO if "tile" in opt else 0
                sources = [("torch", {}), ("seeds", dict(sample_seeds=SEEDS)), ("mix", dict(seed_mix=MIX))]
                for src, kw in sources:
                    run(d, f"chain {tag} {src}", img, s, steps, **kw)
                models.CHAIN_NOISE_BYTES = 2 * B * 3 * H * (W + 2 * hx) * 4
                try:
                    run(d, f"chain {tag} recorded", img, s, steps, noise_fn=keyed_noise(), chain_noise=True)
                finally:
                    models.CHAIN_NOISE_BYTES = budget0
                run(d, f"stepwise {tag} recorded", img, s, steps, noise_fn=keyed_noise())
                if "roi" in opt:
                    for src, kw in sources:
                        run(d, f"stepwise {tag} {src}", img, s, steps, chain_guided=False, **kw)
                bare_loop(d, f"bare {tag}", img, s, steps)
    # the aux stream is passed from Python: C2 dim 160 scale 1 at B = 16, two streams and one
    net, d = build_diffusion("C2", dim=160, device=dev)
    d.omega = 0.3
    H, W = d.image_sizes[1]
    img, d.img_prev_upsample = (hash_randn((16, 3, H, W), 41) * 0.8).to(dev), rnd((16, 3, H, W), 42, 0.5)
    for two in (True, False):
        run(d, f"chain C2 dim160 s1 {H}x{W} B16 two_streams={two} torch", img, 1, STEPS, two_streams=two)
        run(d, f"chain C2 dim160 s1 {H}x{W} B16 two_streams={two} recorded", img, 1, STEPS, two_streams=two,
            noise_fn=keyed_noise(), chain_noise=True)
    # one full pyramid through the public calls
    net, d = build_diffusion("C1", dim=20, device=dev)
    torch.manual_seed(11)
    with scope(d, draw_log=[]):
        img = d.sample(batch_size=2)
        emit("pyramid C1 dim20 scale 0", img)
        for s in range(1, d.n_scales):
            img = d.sample_via_scale(2, img, s)
            emit(f"pyramid C1 dim20 scale {s}", img)
        emit("pyramid C1 dim20 draw_log", img, d.draw_log)
    # drivers: what MultiscaleTrainer's public calls return
    with tempfile.TemporaryDirectory() as tmp:
        tr = c1_trainer(tmp, dev)
        em = tr.ema_model
        H, W = em.image_sizes[-1]
        mask = torch.ones(H, W)
        mask[H // 4:H // 2, W // 3:2 * W // 3] = 0
        ramp, lay = torch.linspace(0, 1, W).expand(H, W).contiguous(), rnd((3, H, W), 70).cpu()
        kw = dict(batch_size=2, seeds=[11, 77], save_images=False)
        roi = dict(target_roi=[10, 12, 30, 40], custom_t_list=em.num_timesteps_ideal[1:], **kw)
        for name, call in [
                ("sample_scales seeds", lambda: tr.sample_scales(**kw)),
                ("sample_scales mix", lambda: tr.sample_scales(batch_size=2, seed_mix=(MIX[0][:2], MIX[1][:2]), save_images=False)),
                ("inpaint", lambda: tr.inpaint(mask, window=None, **kw)),
                ("inpaint window16", lambda: tr.inpaint(mask, window=16, **kw)),
                ("outpaint", lambda: tr.outpaint((1, 1.5), **kw)),
                ("edit ramp", lambda: tr.edit(ramp, **kw)),
                ("paint2image", lambda: tr.paint2image(lay, **kw)),
                ("roi shared", lambda: tr.roi_guided_sampling(roi_bb_list=[[20, 30, 40, 36], [35, 50, 30, 30]], **roi)),
                ("roi per_sample", lambda: tr.roi_guided_sampling(roi_bb_list=[[[20, 30, 40, 36]], [[35, 50, 30, 30]]],
                                                                  per_sample=True, **roi))]:
            torch.manual_seed(13)
            with scope(em, draw_log=[]):
                outs = call()
                for s, y in enumerate(outs):
                    emit(f"drivers {name} scale {s}", y)
                emit(f"drivers {name} draw_log", outs[-1], em.draw_log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
