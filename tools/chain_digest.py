"""SHA-256 digests of what the sampler chain's step tails and the Philox fills compute, to compare two checkouts bit for bit.

    python tools/chain_digest.py [--tree DIR] [--out FILE.txt]

`--tree DIR` imports the package of another checkout (its own library beside its own sources); everything goes through the
C ABI (sinddm_sample_chain_seeds -- the entry with every option -- sinddm_reverse_step / _edit / _keep, sinddm_normal_fill,
sinddm_normal_fill_samples), so one file drives any tree of ABI version 3.  Run it on two trees on ONE box, each in a fresh
process, and compare the outputs line for line (`diff`): a change that is meant to leave the numbers alone must leave every line alone.

For each of the four shapes of tests/test_gpu_chain_guided.py (plain fused tail, padded-row fused tail with and without two
streams, unfused tail) and the batch-of-one unfused shape whose flat tensor ends in a partial quad: every combination of
{edit maps, recorded noise, keep maps} x {per-sample seeds off, on} x {one, two streams}, three steps ending at t = 0, omega =
0.3 (so that sigma is not negligible above the first scale).  Then the stand-alone step in its three modes with and without
edit and keep maps, and both fills at n % 4 in {0, 1, 3}.  The digests depend on the convolution kernels too: they are for
A/B runs, not a fixture."""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import sys

import torch

# (cfg, dim, s, B, steps): tests/test_gpu_chain_guided.SHAPES + the B = 1 shape (3*133*177 % 4 == 3)
SHAPES = [("C2", 160, 0, 16, [700, 2, 0]), ("C2", 160, 1, 16, [400, 1, 0]), ("C2", 160, 3, 4, [311, 2, 0]),
          ("C2", 20, 3, 4, [311, 2, 0]), ("C2", 20, 3, 1, [311, 2, 0])]
FILL_N = [3 * 48 * 64, 3 * 9 * 11, 3 * 133 * 177]             # n % 4 = 0, 1, 3


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("chain_digest.py runs on the GPU: no device found")
    from sinddm_amd import _lib
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.synth import hash_randn
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = _lib.stream_ptr(dev)
    aux_stream = torch.cuda.Stream(dev)
    lines = []

    def emit(name, t):
        lines.append(f"{sha(t)}  {name}")
        print(lines[-1], flush=True)

    def fill(n, seed, sid):
        out = torch.empty(n, device=dev)
        _lib.check(lib.sinddm_normal_fill(_lib.ptr(out), n, seed, sid, st), "sinddm_normal_fill")
        return out

    for cfg, dim, s, B, ts in SHAPES:
        net, d = build_diffusion(cfg, dim=dim, device=dev)
        d.omega = 0.3
        H, W = d.image_sizes[s]
        n = len(ts)
        x0 = (hash_randn((B, 3, H, W), 31 + s) * 0.8).to(dev)
        xt = (hash_randn((B, 3, H, W), 32 + s) * 0.5).clamp(-1, 1).to(dev)
        ew = (hash_randn((H, W), 41) * 0.3 + 0.5).clamp(0, 1).to(dev)           # any affine map  w * x_recon + c
        ec = (hash_randn((3, H, W), 42) * 0.4).to(dev)
        km = (hash_randn((H, W), 43) * 0.6 + 0.5).clamp(0, 1).to(dev)           # mask with exact 0s and 1s and values between
        kx = (hash_randn((3, H, W), 44) * 0.6).clamp(-1, 1).to(dev)
        ab = (C.c_float * (2 * n))(*[v for i in range(n) for v in ((1.0, 0.0) if ts[i] == 0 else (0.8, 0.6))])
        noise = torch.stack([fill(x0.numel(), 4242, 9 + i).view_as(x0) for i in range(n)]).contiguous()
        seeds = torch.tensor([(0x9E3779B97F4A7C15 * (b + 1)) & ((1 << 63) - 1) for b in range(B)], dtype=torch.int64, device=dev)
        coefs = (_lib.StepCoefs * n)(*[d.step_coefs(t, s, True) for t in ts])
        tl = (C.c_int * n)(*ts)
        ws = torch.empty(lib.sinddm_workspace_bytes(dim, B, H, W), dtype=torch.uint8, device=dev)
        for edit, rec, keep, seeded, two in itertools.product([0, 1], repeat=5):
            xa, xb, eps = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
            opts = _lib.ChainOpts()
            if edit:
                opts.edit_w, opts.edit_c = _lib.ptr(ew), _lib.ptr(ec)
            opts.noise = _lib.ptr(noise) if rec else None
            kopts = _lib.KeepOpts()
            kopts.mask, kopts.x0, kopts.ab = _lib.ptr(km), _lib.ptr(kx), C.cast(ab, C.POINTER(C.c_float))
            flag = C.c_int(-1)
            torch.cuda.synchronize()
            _lib.check(lib.sinddm_sample_chain_seeds(
                _lib.ptr(net.flat_params), _lib.ptr(net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
                coefs, tl, n, float(s), 515151 + s, 5, dim, B, H, W, ws.data_ptr(), ws.numel(), st,
                aux_stream.cuda_stream if two else None, C.byref(flag), C.byref(opts), 0, 0, C.byref(kopts) if keep else None,
                _lib.ptr(seeds) if seeded else None), "sinddm_sample_chain_seeds")
            torch.cuda.synchronize()
            y = xb if flag.value == 1 else xa
            if not bool(torch.isfinite(y).all()):
                raise SystemExit("non-finite result")
            emit(f"chain {cfg} dim{dim} s{s} {H}x{W} B{B} edit{edit} noise{rec} keep{keep} seeds{seeded} streams{1 + two}", y)
    # the stand-alone step (sinddm_reverse_step / _edit / _keep): B = 2 samples of 3 x 9 x 11, one step of each mode
    B, HW = 2, 9 * 11
    shp = (B, 3, 9, 11)
    x, e, xb = ((hash_randn(shp, 51 + i) * 0.8).to(dev) for i in range(3))
    ew, ec = (hash_randn((9, 11), 54) * 0.3 + 0.5).clamp(0, 1).to(dev), (hash_randn((3, 9, 11), 55) * 0.4).to(dev)
    km, kx = (hash_randn((9, 11), 56) * 0.6 + 0.5).clamp(0, 1).to(dev), (hash_randn((3, 9, 11), 57) * 0.6).clamp(-1, 1).to(dev)
    z = fill(x.numel(), 99, 1).view(shp)
    for s, t in [(0, 700), (1, 400), (1, 0)]:
        k, out = d.step_coefs(t, s, True), torch.empty_like(x)
        p = [_lib.ptr(v) for v in (x, e, xb, z, out)] + [C.byref(k)]
        _lib.check(lib.sinddm_reverse_step(*p, x.numel(), st), "sinddm_reverse_step")
        emit(f"reverse_step mode{k.mode}", out)
        _lib.check(lib.sinddm_reverse_step_edit(*p, _lib.ptr(ew), _lib.ptr(ec), B, 3, HW, st), "sinddm_reverse_step_edit")
        emit(f"reverse_step_edit mode{k.mode}", out)
        for name, w, c in (("keep", None, None), ("keep_edit", ew, ec)):
            _lib.check(lib.sinddm_reverse_step_keep(*p, _lib.ptr(w), _lib.ptr(c), _lib.ptr(km), _lib.ptr(kx), 0.8, 0.6, B, 3, HW,
                                                    st), "sinddm_reverse_step_keep")
            emit(f"reverse_step_{name} mode{k.mode}", out)
    for n in FILL_N:
        emit(f"normal_fill n{n}", fill(n, 777, 3))
        B = 5
        seeds = torch.tensor([0, (1 << 63) - 1, 12345, 12345, 0x0123456789ABCDEF], dtype=torch.int64, device=dev)
        out = torch.empty(B * n, device=dev)
        _lib.check(lib.sinddm_normal_fill_samples(_lib.ptr(out), B, n, _lib.ptr(seeds), 3, st), "sinddm_normal_fill_samples")
        emit(f"normal_fill_samples B{B} n{n}", out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
