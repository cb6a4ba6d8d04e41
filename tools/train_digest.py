"""SHA-256 digests of what the training step's PYTHON route computes, to compare two checkouts bit for bit.

    python tools/train_digest.py [--tree DIR] [--out FILE.txt]

The training twin of tools/run_digest.py: `--tree DIR` imports the package of another checkout (its own library beside its own
sources).  Run it on two trees on ONE box, each in a fresh process, and `diff` the outputs: a change of the host side that is
meant to leave the numbers alone must leave every line alone.

One `MultiScaleGaussianDiffusion.p_losses` + `backward()` per case on C1 at dim 16 (He-normal weights), B = 2: every combination
of the loss type, `train_tile` {off, x, y, xy}, `train_weights` {None, a soft map, a map with a hole}, the scale {0, 1, 2}, t[0]
{0, > 0: the host-synchronised branch of 'l1_pred_img'} and the shape {7x12, 9x33: W % 4 != 0}.  A line is the digest of
x_noisy, of the network's output and of the gradient handed to the network's backward (a forward hook on the network).  The
loss's own bits are in the digest only where it is the sum of at most two workgroups' partial sums, which commutes: untiled 'l1'
with B*3*H*W <= 512, untiled weighted 'l1' with <= 1024; elsewhere the order of the atomics varies from run to run (the tests hold
it to 1e-5 of float64).  The flat gradient buffer is not reproducible run to run and stays out
(tests/test_gpu_tile_train.py::test_off_is_the_untouched_step).  The digests depend on the kernels too: for A/B runs, not a
fixture."""
import argparse
import hashlib
import itertools
import os
import sys

import torch

B = 2
TILES = {"off": (False, False), "x": (False, True), "y": (True, False), "xy": (True, True)}


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p.detach().cpu().contiguous().numpy().tobytes() if isinstance(p, torch.Tensor) else repr(p).encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("train_digest.py runs on the GPU: no device found")
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.synth import hash_randn, he_state_dict
    dev, lines = torch.device("cuda:0"), []
    net, d = build_diffusion("C1", dim=16, device=dev)
    net.load_state_dict(he_state_dict(16))
    rec = {}

    def hook(mod, inp, out):
        rec["x_noisy"], rec["eps"] = inp[0].detach().clone(), out.detach().clone()
        out.register_hook(lambda g: rec.__setitem__("grad_eps", g.detach().clone()))

    net.register_forward_hook(hook)

    def weight_map(kind, H, W):
        if kind == "none":
            return None
        if kind == "soft":
            return hash_randn((H, W), 21 + W).abs().mul(0.5).clamp(0.05, 1).to(dev).contiguous()
        w = torch.ones(H, W)
        w[H // 3:H // 3 + 3, W // 4:W // 4 + 4] = 0.0
        return w.to(dev)

    for (H, W), lt, tile, kind, s, t0 in itertools.product(((7, 12), (9, 33)), ("l1", "l2", "l1_pred_img"), TILES,
                                                           ("none", "soft", "hole"), (0, 1, 2), (0, 7)):
        x_start, x_orig = ((hash_randn((B, 3, H, W), 31 + k) * 0.5).clamp(-1, 1).to(dev) for k in range(2))
        noise, t = hash_randn((B, 3, H, W), 33).to(dev), torch.tensor([t0, 31], device=dev)
        w = weight_map(kind, H, W)
        d.loss_type, d.train_tile, d.train_weights = lt, TILES[tile], [w] * d.n_scales if w is not None else None
        net.bind_grads()
        net.flat_grads.zero_()
        rec.clear()
        loss = d.p_losses(x_start, t, s, noise=noise, **(dict(x_orig=x_orig) if s > 0 else {}))
        loss.backward()
        torch.cuda.synchronize()
        parts = [rec["x_noisy"], rec["eps"], rec["grad_eps"]]
        if not all(bool(torch.isfinite(v).all()) for v in parts + [loss]):
            raise SystemExit(f"non-finite result: {lt} {tile} {kind} s{s} t0={t0} {H}x{W}")
        with_loss = lt == "l1" and tile == "off" and B * 3 * H * W <= (512 if w is None else 1024)
        if with_loss:
            parts.append(loss)
        lines.append(f"{sha(*parts)}  {H}x{W} {lt} tile={tile} weights={kind} s{s} t0={t0}{' +loss' if with_loss else ''}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
