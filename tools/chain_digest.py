"""SHA-256 digests of what the sampler chain's step tails and the Philox fills compute, to compare two checkouts bit for bit.

    python tools/chain_digest.py [--tree DIR] [--out FILE.txt]

`--tree DIR` imports the package of another checkout (its own library beside its own sources); everything goes through the
C ABI (sinddm_sample_chain_seeds, sinddm_sample_chain_solver, the sinddm_reverse_step* entries, sinddm_layout_delta,
sinddm_normal_fill, sinddm_normal_fill_samples), so one file drives any tree of ABI version 3 that has these entries.  Run it
on two trees on ONE box, each in a fresh process, and compare the outputs line for line (`diff`): a change that is meant to
leave the numbers alone must leave every line alone.

For each of the four shapes of tests/test_gpu_chain_guided.py (plain fused tail, padded-row fused tail with and without two
streams, unfused tail) and the batch-of-one unfused shape whose flat tensor ends in a partial quad: every combination of
{edit maps, recorded noise, keep maps} x {per-sample seeds off, on} x {one, two streams}, three steps ending at t = 0, omega =
0.3 (so that sigma is not negligible above the first scale).  Then the stand-alone step in its three modes with and without
edit and keep maps, and both fills at n % 4 in {0, 1, 3}.

The three tail forms on the stream-row walk (jump, layout pull, multistep), still through the C ABI alone:
  * their single-step entries (sinddm_reverse_step_jump, sinddm_layout_delta + sinddm_reverse_step_layout,
    sinddm_reverse_step_ms) on B = 2 samples of 3 x 5 x 7 (3 H W % 4 == 1: a quad crosses the sample's end, the last quad is
    partial) and 3 x 8 x 12 (every quad full and aligned), modes 0 and 1 (for _ms also a landing in mode 2 with q == 0) x
    {edit off, on} x {keep off, on}; layout with block sizes 1 and 3 (3 divides neither centre), without and with a wrapped
    halo; _ms with q == 0 and q != 0, the history as well as the output;
  * three-step chains through sinddm_sample_chain_solver -- the entry with every option -- with a resample block that jumps,
    a layout block that pulls, a solver block of order 2: the shapes above (the padded-row shape with one and two streams)
    and C2 dim 160 scale 1 at B = 18 on two streams, whose second half starts inside a quad of the batch's stream, x
    {edit maps off, on} x {keep maps off, on} x {per-sample seeds off, on} x {recorded noise off, on} (the jumps then read
    a buffer of their own); and each form once with per-sample maps (sinddm_batch_opts) on the unfused B = 4 shape, where a
    quad runs into the next sample's slices.
The digests depend on the convolution kernels too: they are for A/B runs, not a fixture."""
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
# the stream counts of the form chains per shape of SHAPES, and the shape whose second half starts inside a quad (two streams:
# 9 * 3 * 67 * 90 % 4 == 2); it runs the form chains alone
FORM_STREAMS = [(1,), (1, 2), (1,), (1,), (1,)]
UNALIGNED_HALF = ("C2", 160, 1, 18, [400, 1, 0])
FORMS = ("jump", "layout", "ms")


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

    def form_blocks(form, coefs, n, B, H, W, rec, per_sample, keepalive):
        """The (rs, lo, so) blocks of a three-step chain in which every step that may ends in `form`; `keepalive` takes what
        the blocks point to, the multistep history first."""
        rs = lo = so = None
        if form == "jump":                                   # (never after a mode-2 step; d only where x-tilde is read)
            jumps = (_lib.JumpCoefs * n)(*[_lib.JumpCoefs(int(k.mode != 2), 0.9, 0.19 ** 0.5, 0.05 if k.mode == 1 else 0.0)
                                          for k in coefs])
            jnz = torch.stack([fill(B * 3 * H * W, 2424, 40 + i) for i in range(n)]).contiguous() if rec else None
            rs = _lib.ResampleOpts(jumps, _lib.ptr(jnz))
            keepalive += [None, jumps, jnz]
        elif form == "layout":
            down = 5
            lay = (hash_randn((B if per_sample else 1, 3, H, W), 45) * 0.5).to(dev)
            g = (C.c_float * n)(0.5, 0.25, 0.125)
            delta = torch.empty(B * 3 * (-(-H // down)) * (-(-W // down)), device=dev)
            lo = _lib.LayoutOpts(_lib.ptr(lay), down, C.cast(g, C.POINTER(C.c_float)), _lib.ptr(delta))
            keepalive += [None, lay, g, delta]
        else:
            q = (C.c_float * n)(*[0.0 if i == 0 or k.mode == 2 else 0.35 for i, k in enumerate(coefs)])
            hist = torch.full((B, 3, H, W), float("nan"), device=dev)       # (a step reads it only after one has written it)
            so = _lib.SolverOpts(C.cast(q, C.POINTER(C.c_float)), _lib.ptr(hist))
            keepalive += [hist, q]
        return rs, lo, so

    for si, (cfg, dim, s, B, ts) in enumerate(SHAPES + [UNALIGNED_HALF]):
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
        base = [_lib.ptr(net.flat_params), _lib.ptr(net.packed_weights())]

        def chain(edit, rec, keep, seeded, two, form=None, per_sample=False):
            """One chain call: sinddm_sample_chain_seeds, or with a `form` sinddm_sample_chain_solver; the result (and the
            multistep history) go to the digest."""
            xa, xb, eps = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
            maps = [ew, ec, km, kx]
            if per_sample:                                   # (sample b's slice: the shared map times a factor of its own)
                maps = [(m.unsqueeze(0) * torch.linspace(0.6, 1.0, B, device=dev).view(B, *[1] * m.dim())).contiguous() for m in maps]
            opts = _lib.ChainOpts()
            if edit:
                opts.edit_w, opts.edit_c = _lib.ptr(maps[0]), _lib.ptr(maps[1])
            opts.noise = _lib.ptr(noise) if rec else None
            kopts = _lib.KeepOpts()
            kopts.mask, kopts.x0, kopts.ab = _lib.ptr(maps[2]), _lib.ptr(maps[3]), C.cast(ab, C.POINTER(C.c_float))
            flag = C.c_int(-1)
            args = base + [_lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt), coefs, tl, n, float(s), 515151 + s, 5, dim, B, H, W,
                           ws.data_ptr(), ws.numel(), st, aux_stream.cuda_stream if two else None, C.byref(flag), C.byref(opts), 0, 0,
                           C.byref(kopts) if keep else None, _lib.ptr(seeds) if seeded else None]
            name = f"{cfg} dim{dim} s{s} {H}x{W} B{B} edit{edit} noise{rec} keep{keep} seeds{seeded} streams{1 + two}"
            held = []
            torch.cuda.synchronize()
            if form is None:
                _lib.check(lib.sinddm_sample_chain_seeds(*args), "sinddm_sample_chain_seeds")
                name = "chain " + name
            else:
                rs, lo, so = form_blocks(form, coefs, n, B, H, W, rec, per_sample, held)
                gain = torch.linspace(0.5, 1.0, B, device=dev)
                bo = None
                if per_sample:                               # (the layout fields only beside a layout block)
                    bo = _lib.BatchOpts(edit, keep, keep, int(form == "layout"), _lib.ptr(gain) if form == "layout" else None)
                _lib.check(lib.sinddm_sample_chain_solver(*args, C.byref(rs) if rs else None, C.byref(lo) if lo else None,
                                                          C.byref(bo) if bo else None, C.byref(so) if so else None),
                           "sinddm_sample_chain_solver")
                name = f"chain_{form} {name}" + (" per_sample_maps" if per_sample else "")
            torch.cuda.synchronize()
            y = xb if flag.value == 1 else xa
            if not bool(torch.isfinite(y).all()):
                raise SystemExit("non-finite result")
            emit(name, y)
            if form == "ms":
                emit(name + " hist", held[0])

        if si < len(SHAPES):
            for edit, rec, keep, seeded, two in itertools.product([0, 1], repeat=5):
                chain(edit, rec, keep, seeded, two)
        for form, streams, edit, keep, seeded, rec in itertools.product(FORMS, FORM_STREAMS[si] if si < len(SHAPES) else (2,),
                                                                        *[[0, 1]] * 4):
            chain(edit, rec, keep, seeded, streams - 1, form)
        if (cfg, dim, s, B) == ("C2", 20, 3, 4):             # unfused, B >= 2: a quad crosses into the next sample's slices
            for form in FORMS:
                chain(1, 0, 1, 0, 0, form, per_sample=True)
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
    # the single-step entries of the three forms: B = 2 samples of 3 x 5 x 7 and 3 x 8 x 12 (the buffers' size)
    B = 2
    for H, W in [(5, 7), (8, 12)]:
        shp, HW = (B, 3, H, W), H * W
        x, e, xb, hist0 = ((hash_randn(shp, 61 + i) * 0.8).to(dev) for i in range(4))
        ew, ec = (hash_randn((H, W), 65) * 0.3 + 0.5).clamp(0, 1).to(dev), (hash_randn((3, H, W), 66) * 0.4).to(dev)
        km, kx = (hash_randn((H, W), 67) * 0.6 + 0.5).clamp(0, 1).to(dev), (hash_randn((3, H, W), 68) * 0.6).clamp(-1, 1).to(dev)
        lay = (hash_randn((3, H, W), 69) * 0.5).to(dev)
        z, z2 = fill(x.numel(), 99, 1).view(shp), fill(x.numel(), 99, 2).view(shp)
        for (s, t), edit, keep in itertools.product([(0, 700), (1, 400), (1, 0)], [0, 1], [0, 1]):
            k, out = d.step_coefs(t, s, True), torch.empty_like(x)
            maps = [_lib.ptr(ew) if edit else None, _lib.ptr(ec) if edit else None, _lib.ptr(km) if keep else None,
                    _lib.ptr(kx) if keep else None, 0.8, 0.6]
            tag = f"{H}x{W} mode{k.mode} edit{edit} keep{keep}"
            for q in (0.0, 0.35):
                if q != 0.0 and k.mode == 2:
                    continue
                hist = hist0.clone()
                _lib.check(lib.sinddm_reverse_step_ms(*[_lib.ptr(v) for v in (x, e, xb, z, out)], C.byref(k), q, _lib.ptr(hist), *maps, B,
                                                      3, HW, st), "sinddm_reverse_step_ms")
                emit(f"reverse_step_ms {tag} q{q}", out)
                emit(f"reverse_step_ms {tag} q{q} hist", hist)
            if k.mode == 2:                                  # (only the multistep step lands in mode 2 here)
                continue
            jc = _lib.JumpCoefs(1, 0.9, 0.19 ** 0.5, 0.05 if k.mode == 1 else 0.0)
            _lib.check(lib.sinddm_reverse_step_jump(*[_lib.ptr(v) for v in (x, e, xb, z, z2, out)], C.byref(k), C.byref(jc), *maps, B, 3,
                                                    HW, st), "sinddm_reverse_step_jump")
            emit(f"reverse_step_jump {tag}", out)
            for down, hx in itertools.product([1, 3], [0, 2]):       # (hx: a wrapped halo of 2 columns inside the same buffers)
                Wc = W - 2 * hx
                delta = torch.empty(B * 3 * (-(-H // down)) * (-(-Wc // down)), device=dev)
                _lib.check(lib.sinddm_layout_delta(*[_lib.ptr(v) for v in (x, e, xb, lay, delta)], C.byref(k), maps[0], maps[1], down, B,
                                                   H, Wc, 0, hx, st), "sinddm_layout_delta")
                emit(f"layout_delta {tag} down{down} halo{hx}", delta)
                _lib.check(lib.sinddm_reverse_step_layout(*[_lib.ptr(v) for v in (x, e, xb, z, out)], C.byref(k), _lib.ptr(delta), 0.5,
                                                          down, *maps, B, H, Wc, 0, hx, 0, int(hx != 0), st),
                           "sinddm_reverse_step_layout")
                emit(f"reverse_step_layout {tag} down{down} halo{hx}", out)
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
