#!/usr/bin/env python3
"""Time sinddm_patch_nnf against a torch formulation of the same result on the same GPU, in one process, alternating.

    python tools/nnf_bench.py [--runs 7] [--patch 7] [--shapes 16x186x248 16x48x64] [--lib tools/ab/libnnf_x.so ...]
                              [--scaled] [--vote] [--no-torch] [--local 4 8 16]

Per shape B x H x W (query and reference of the same size, one shared reference) every route is warmed up once and then
timed `--runs` times in turn (route A, route B, route A, ...) with device events; the report is the median, the min .. max
spread, and for the library routes the share of the 157.3 TF/s fp32 matrix peak counted as 2 M N K_pad.  `--lib` adds
variant builds of csrc/patch_nnf.hip (the translation unit stands alone:
`hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I include -DSINDDM_NNF_QB=2 sinddm_amd/csrc/patch_nnf.hip -o x.so`).
The torch route: F.unfold of both images, then per sample and per chunk of queries addmm(|b|^2, A, B, alpha=-2) and min over
the references -- the M x N matrix goes through HBM chunk by chunk.  Its distances are compared with the library's first.
`--scaled` adds the library's sinddm_patch_nnf_scaled with a random scale map in [0.5, 2) (same FLOP count); `--vote` adds
sinddm_patch_vote on the library's own field and a device copy of the bytes the vote streams (the field, base and out:
28 bytes per pixel; the gathered reference reads are not counted), both reported in GB/s.  `--local R ...` adds, per radius,
sinddm_patch_nnf_local with a coherent prior (the identity field plus a jitter of -1 .. 1 per axis) and with a random prior,
in turn with the exhaustive route of the same process; they report candidate pairs per second, B M (2R + 1)^2 / time, and
the share of their winners that are the exhaustive route's."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sinddm_amd import _lib  # noqa: E402

PEAK_TFLOPS = 157.3


def bind(path):
    lib = C.CDLL(path)
    p, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.sinddm_patch_nnf_workspace_bytes.restype, lib.sinddm_patch_nnf_workspace_bytes.argtypes = sz, [i] * 8
    lib.sinddm_patch_nnf.restype = i
    lib.sinddm_patch_nnf.argtypes = [p, i, p, i, p, p, p, i, i, i, i, i, i, i, i, p, sz, p]
    if hasattr(lib, "sinddm_patch_nnf_scaled"):                 # (a variant build of an older source has neither)
        lib.sinddm_patch_nnf_scaled_workspace_bytes.restype, lib.sinddm_patch_nnf_scaled_workspace_bytes.argtypes = sz, [i] * 8
        lib.sinddm_patch_nnf_scaled.restype = i
        lib.sinddm_patch_nnf_scaled.argtypes = [p, i, p, i, p, p, i, p, p, i, i, i, i, i, i, i, i, p, sz, p]
        lib.sinddm_patch_vote.restype = i
        lib.sinddm_patch_vote.argtypes = [p, p, i, p, p, i, p, i, i, i, i, i, i, i, i, C.c_float, p]
    if hasattr(lib, "sinddm_patch_nnf_local"):
        lib.sinddm_patch_nnf_local.restype = i
        lib.sinddm_patch_nnf_local.argtypes = [p, i, p, i, p, p, i, p, i, p, p, i, i, i, i, i, i, i, i, p]
    return lib


def lib_route(lib, q, r, P):
    B, _, H, W = q.shape
    Hr, Wr = r.shape[2:]
    n = lib.sinddm_patch_nnf_workspace_bytes(B, H, W, Hr, Wr, P, 0, 0)
    ws = torch.empty(n, dtype=torch.uint8, device=q.device)
    dist = torch.empty(B, H - P + 1, W - P + 1, device=q.device)
    idx = torch.empty(B, H - P + 1, W - P + 1, dtype=torch.int32, device=q.device)

    def run():
        rc = lib.sinddm_patch_nnf(q.data_ptr(), 1, r.data_ptr(), 0, None, dist.data_ptr(), idx.data_ptr(), B, H, W, Hr, Wr, P, 0,
                                  0, ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return dist, idx
    return run


def scaled_route(lib, q, r, P):
    B, _, H, W = q.shape
    Hr, Wr = r.shape[2:]
    n = lib.sinddm_patch_nnf_scaled_workspace_bytes(B, H, W, Hr, Wr, P, 0, 0)
    ws = torch.empty(n, dtype=torch.uint8, device=q.device)
    dist = torch.empty(B, H - P + 1, W - P + 1, device=q.device)
    idx = torch.empty(B, H - P + 1, W - P + 1, dtype=torch.int32, device=q.device)
    g = torch.Generator(device="cpu").manual_seed(2)
    scale = (torch.rand(1, Hr - P + 1, Wr - P + 1, generator=g) * 1.5 + 0.5).to(q.device)

    def run():
        rc = lib.sinddm_patch_nnf_scaled(q.data_ptr(), 1, r.data_ptr(), 0, None, scale.data_ptr(), 0, dist.data_ptr(),
                                         idx.data_ptr(), B, H, W, Hr, Wr, P, 0, 0, ws.data_ptr(), n,
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return dist, idx
    return run


def local_priors(B, h, w, device):
    """(coherent: the identity field plus a jitter of -1 .. 1 per axis, clamped into the grid; random), (B, h, w) int32."""
    g = torch.Generator(device="cpu").manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    jy, jx = torch.randint(-1, 2, (B, h, w), generator=g), torch.randint(-1, 2, (B, h, w), generator=g)
    coherent = (yy[None] + jy).clamp(0, h - 1) * w + (xx[None] + jx).clamp(0, w - 1)
    rand = torch.randint(0, h * w, (B, h, w), generator=g)
    return coherent.to(torch.int32).to(device), rand.to(torch.int32).to(device)


def local_route(lib, q, r, P, radius, prior):
    B, _, H, W = q.shape
    Hr, Wr = r.shape[2:]
    dist = torch.empty(B, H - P + 1, W - P + 1, device=q.device)
    idx = torch.empty(B, H - P + 1, W - P + 1, dtype=torch.int32, device=q.device)

    def run():
        rc = lib.sinddm_patch_nnf_local(q.data_ptr(), 1, r.data_ptr(), 0, None, None, 0, prior.data_ptr(), radius, dist.data_ptr(),
                                        idx.data_ptr(), B, H, W, Hr, Wr, P, 0, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return dist, idx
    return run


def vote_routes(lib, q, r, P, idx):
    """(the vote on the field `idx`, a copy of as many bytes as the vote streams)."""
    B, _, H, W = q.shape
    Hr, Wr = r.shape[2:]
    out = torch.empty_like(q)
    nbytes = idx.numel() * 4 + 2 * q.numel() * 4
    src = torch.empty(nbytes // 8, dtype=torch.float32, device=q.device)
    dst = torch.empty_like(src)

    def vote():
        rc = lib.sinddm_patch_vote(idx.data_ptr(), r.data_ptr(), 0, q.data_ptr(), None, 0, out.data_ptr(), B, H, W, Hr, Wr, P, 0,
                                   0, 1.0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out, idx

    def copy():
        dst.copy_(src)
        return dst, idx
    return vote, copy, nbytes


def torch_route(q, r, P, chunk_bytes=1 << 30):
    B = q.shape[0]
    Bm = F.unfold(r, P)[0].contiguous()                         # (K, N)
    nb = (Bm * Bm).sum(dim=0)
    N = Bm.shape[1]
    rows = max(256, chunk_bytes // (4 * N))

    def run():
        dists, idxs = [], []
        for b in range(B):
            A = F.unfold(q[b:b + 1], P)[0].t()                  # (M, K)
            na = (A * A).sum(dim=1)
            d_parts, i_parts = [], []
            for m0 in range(0, A.shape[0], rows):
                a = A[m0:m0 + rows]
                rank = torch.addmm(nb[None, :].expand(a.shape[0], N), a, Bm, alpha=-2.0)
                v, i = rank.min(dim=1)
                d_parts.append(v + na[m0:m0 + rows])
                i_parts.append(i)
            dists.append(torch.cat(d_parts))
            idxs.append(torch.cat(i_parts))
        return torch.stack(dists), torch.stack(idxs)
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--patch", type=int, default=7)
    ap.add_argument("--shapes", nargs="+", default=["16x186x248", "16x48x64"])
    ap.add_argument("--lib", nargs="*", default=[])
    ap.add_argument("--scaled", action="store_true")
    ap.add_argument("--vote", action="store_true")
    ap.add_argument("--no-torch", dest="torch", action="store_false")
    ap.add_argument("--local", type=int, nargs="*", default=[], metavar="R")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.load()
    libs = [("library", bind(_lib.LIB_PATH))] + [(os.path.basename(p), bind(p)) for p in args.lib]
    P = args.patch
    kpad = (3 * P * P + 3) // 4 * 4
    for shape in args.shapes:
        B, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cpu").manual_seed(1)
        q = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(dev)
        r = (torch.rand(1, 3, H, W, generator=g) * 2 - 1).to(dev)
        routes = [(name, lib_route(lib, q, r, P)) for name, lib in libs]
        if args.torch:
            routes.append(("torch", torch_route(q, r, P)))
        outs = {name: tuple(t.clone() for t in run()) for name, run in routes}      # warm-up, and the results to compare
        moved = {}                                                                  # bytes of the routes reported in GB/s
        if args.scaled:
            routes.append(("scaled", scaled_route(libs[0][1], q, r, P)))
        if args.vote:
            vote, copy, nbytes = vote_routes(libs[0][1], q, r, P, outs["library"][1])
            routes += [("vote", vote), ("copy", copy)]
            moved = {"vote": nbytes, "copy": nbytes}
        pairs, agree = {}, {}
        if args.local:
            coherent, rand = local_priors(B, H - P + 1, W - P + 1, dev)
            for radius in args.local:
                for kind, prior in (("coherent", coherent), ("random", rand)):
                    name = f"local R={radius} {kind}"
                    run = local_route(libs[0][1], q, r, P, radius, prior)
                    routes.append((name, run))
                    pairs[name] = B * (H - P + 1) * (W - P + 1) * (2 * radius + 1) ** 2
                    agree[name] = float((run()[1] == outs["library"][1]).float().mean())
        for name, run in routes[len(outs):]:
            run()
        torch.cuda.synchronize()
        d0 = outs["library"][0].reshape(B, -1)
        for name, (d, _) in outs.items():
            err = float((d.reshape(B, -1) - d0).abs().max())
            print(f"# {shape} {name}: max |dist - library dist| {err:.3e} (dist up to {float(d0.max()):.3e})", flush=True)
        times = {name: [] for name, _ in routes}
        for _ in range(args.runs):
            for name, run in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        M = N = (H - P + 1) * (W - P + 1)
        flop = 2.0 * B * M * N * kpad
        for name, ts in times.items():
            med = statistics.median(ts)
            if name in moved:
                print(json.dumps({"shape": shape, "patch": P, "route": name, "runs": len(ts), "median_ms": round(med, 4),
                                  "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "bytes": moved[name],
                                  "gb_per_s": round(moved[name] / med * 1e-6, 1)}), flush=True)
                continue
            if name in pairs:
                print(json.dumps({"shape": shape, "patch": P, "route": name, "runs": len(ts), "median_ms": round(med, 4),
                                  "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "pairs": pairs[name],
                                  "gpairs_per_s": round(pairs[name] / med * 1e-6, 2),
                                  "winners_equal_exhaustive": round(agree[name], 4)}), flush=True)
                continue
            rec = {"shape": shape, "patch": P, "route": name, "runs": len(ts), "median_ms": round(med, 4), "min_ms": round(min(ts), 4),
                   "max_ms": round(max(ts), 4), "tflops": round(flop / med * 1e-9, 2),
                   "peak_share": round(flop / med * 1e-9 / PEAK_TFLOPS, 4)}
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
