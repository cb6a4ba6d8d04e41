"""SHA-256 digests of what the network's 3x3 conv routes compute and launch, to compare two checkouts bit for bit.

    python tools/net_digest.py [--tree DIR] [--out FILE.txt] [--grads FILE.pt]
    python tools/net_digest.py --compare A.pt B.pt

`--tree DIR` imports the package of another checkout (its own library beside its own sources); everything goes through the
C ABI of version 3 and the three one-number route hooks every such tree has, so one file drives any of them.  Run it on two
trees on ONE box, each in a fresh process, and `diff` the outputs: a refactor of the routing / packing / launch code must
leave every line alone.

Lines, in this order:
  * `routes ...`: sinddm_debug_conv_path / _infer_path / _train_path / _head_path over the grid of tests/test_routes_host.py
    (one digest per width, and the row count), and -- only where the tree has sinddm_debug_wgrad_routes -- the 17
    weight-gradient launches over the same grid at 256, 64 and 304 CUs.  Without a device the tool stops here (the hooks
    then assume 256 CUs).
  * both packed buffers (zero-filled before packing, so the alignment gaps do not differ) at dims 160, 80, 32, 20, 10;
  * sinddm_net_forward on closed-form and He weights at one shape per route;
  * y and grad_x of sinddm_net_forward_train + sinddm_net_backward (the parameter gradients go through atomics: the suite
    gates them, a digest cannot);
  * per shape, the launch counts per (kind, generation) of the conv profiler.
`--grads` saves the flat parameter gradients of the TRAIN shapes; `--compare` prints, per shape, the worst per-tensor rel-L2
distance between two such files (two runs of one tree give the run-to-run noise of the atomics: the suite's bound is 2e-6).
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch

DIMS = (10, 16, 20, 28, 32, 48, 80, 160, 240)
BATCHES = (1, 2, 4, 16, 32, 64)
SIZES = ((9, 11), (20, 20), (30, 30), (48, 64), (67, 90), (76, 95), (96, 128), (99, 130), (116, 145), (133, 177), (186, 248),
         (411, 512))
FP32 = 0x10000                                   # SINDDM_DIM_FP32_CONVS
PACK_DIMS = (160, 80, 32, 20, 10)
# (dim, fp32_convs, B, H, W): wh, wino4, padded rows, wino3, wino2, dim 80 (fp32 conv1 in front of a conv_wh conv2), direct kernels
FORWARD = [(160, 0, 32, 96, 128), (160, 1, 32, 96, 128), (160, 0, 28, 99, 130), (160, 0, 16, 48, 64), (160, 0, 1, 20, 20),
           (80, 0, 16, 186, 248), (20, 0, 4, 133, 177), (10, 0, 4, 30, 30)]
TRAIN = [(160, 0, 32, 96, 128), (160, 1, 32, 96, 128), (32, 0, 2, 30, 30)]
KINDS = [(1, g) for g in (2, 3, 4, 8)] + [(2, 0), (3, 0), (4, 0), (4, 8)]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def sha_t(t):
    return sha(t.detach().cpu().contiguous().numpy().tobytes())


def route_rows(lib):
    """The four old hooks over the whole grid: {dim_arg: [(B, H, W, conv, infer, train, head), ...]}."""
    table = {}
    for dim in DIMS:
        for da in (dim, dim | FP32):
            table[da] = [(B, H, W, lib.sinddm_debug_conv_path(da, B, H, W), lib.sinddm_debug_infer_path(da, B, H, W),
                          lib.sinddm_debug_train_path(da, B, H, W), lib.sinddm_debug_head_path(da, B, H, W))
                         for B in BATCHES for H, W in SIZES]
    return table


def compare(a_path, b_path, net_param_shapes):
    a, b = torch.load(a_path), torch.load(b_path)
    worst_all = 0.0
    for tag in a:
        dim, off, worst = int(tag.split()[0][3:]), 0, (0.0, "")
        for name, shape in net_param_shapes(dim).items():
            n = 1
            for v in shape:
                n *= v
            x, y = a[tag][off:off + n].double(), b[tag][off:off + n].double()
            worst = max(worst, (float((x - y).norm() / y.norm().clamp_min(1e-300)), name))
            off += n
        assert off == a[tag].numel() == b[tag].numel()
        worst_all = max(worst_all, worst[0])
        print(f"flat_grads {tag}: worst per-tensor rel-L2 {worst[0]:.3e} ({worst[1]})")
    print(f"flat_grads worst {worst_all:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--grads", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if args.compare:
        from sinddm_amd.synth import net_param_shapes
        return compare(*args.compare, net_param_shapes)
    from sinddm_amd import _lib
    from sinddm_amd.synth import closed_form_state_dict, hash_randn, he_state_dict, net_param_shapes
    lib = _lib.load()
    lines = []

    def emit(name, digest):
        lines.append(f"{digest}  {name}")
        print(lines[-1], flush=True)

    def finish():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    rows = 0
    for da, tab in route_rows(lib).items():
        rows += len(tab)
        emit(f"routes dim{da & 0xFFFF} fp32_convs{int(bool(da & FP32))} rows{len(tab)}", sha(repr(tab).encode()))
    emit(f"routes rows compared {rows}", sha(b""))
    if hasattr(lib, "sinddm_debug_wgrad_routes"):
        for ncu in (256, 64, 304):
            tab = []
            for dim in DIMS:
                for da in (dim, dim | FP32):
                    for B in BATCHES:
                        for H, W in SIZES:
                            out = (C.c_int * 68)()
                            _lib.check(lib.sinddm_debug_wgrad_routes(da, B, H, W, ncu, out, 68), "sinddm_debug_wgrad_routes")
                            tab.append((da, B, H, W, list(out)))
            emit(f"wgrad routes ncu{ncu} rows{len(tab)}", sha(repr(tab).encode()))
    if not torch.cuda.is_available():
        print("no device: route tables only", flush=True)
        finish()
        return

    dev = torch.device("cuda:0")
    st = _lib.stream_ptr(dev)

    def flat(sd, dim):
        return torch.cat([sd[k].reshape(-1).float() for k in net_param_shapes(dim)]).to(dev).contiguous()

    def packed(params, dim, bwd=False):
        n = (lib.sinddm_packed_bwd_count if bwd else lib.sinddm_packed_count)(dim)
        buf = torch.zeros(n, device=dev)
        fn = lib.sinddm_pack_weights_bwd if bwd else lib.sinddm_pack_weights
        _lib.check(fn(_lib.ptr(params), _lib.ptr(buf), dim, st), "pack")
        torch.cuda.synchronize()
        return buf

    weights = {}

    def net(dim, fill):
        if (dim, fill) not in weights:
            p = flat(closed_form_state_dict(dim) if fill == "closed" else he_state_dict(dim), dim)
            weights[(dim, fill)] = (p, packed(p, dim), packed(p, dim, bwd=True))
        return weights[(dim, fill)]

    def launches():
        """the profiler's launch count per (kind, generation) since sinddm_prof_begin, as text"""
        out = []
        for kind, gen in KINDS:
            n = C.c_int64(0)
            _lib.check(lib.sinddm_prof_end3(10 * kind + gen if gen else kind, None, C.byref(n), None, None, 0), "prof_end3")
            out.append(f"k{kind}g{gen}={n.value}")
        _lib.check(lib.sinddm_prof_end3(0, None, None, None, None, 1), "prof_end3")
        return " ".join(out)

    for dim in PACK_DIMS:
        for fill in ("closed", "he"):
            _, pk, pkb = net(dim, fill)
            emit(f"packed dim{dim} {fill}", sha_t(pk))
            emit(f"packed_bwd dim{dim} {fill}", sha_t(pkb))

    for dim, fp32, B, H, W in FORWARD:
        da = dim | (FP32 if fp32 else 0)
        x = (hash_randn((B, 3, H, W), 700 + W) * 0.9).to(dev)
        t = torch.tensor([(53 * (i + 3)) % 1000 for i in range(B)], dtype=torch.long, device=dev)
        ws = torch.empty(lib.sinddm_workspace_bytes(da, B, H, W), dtype=torch.uint8, device=dev)
        tag = f"dim{dim} fp32_convs{fp32} {B}x{H}x{W}"
        for fill in ("closed", "he"):
            p, pk, _ = net(dim, fill)
            out = torch.empty(B, 3, H, W, device=dev)
            _lib.check(lib.sinddm_prof_begin(), "prof_begin")
            _lib.check(lib.sinddm_net_forward(_lib.ptr(p), _lib.ptr(pk), _lib.ptr(x), _lib.ptr(t), 0, 2.0, _lib.ptr(out), da, B, H, W,
                                              ws.data_ptr(), ws.numel(), st), "sinddm_net_forward")
            torch.cuda.synchronize()
            counts = launches()
            if not bool(torch.isfinite(out).all()):
                raise SystemExit("non-finite result")
            emit(f"forward {tag} {fill}", sha_t(out))
        emit(f"forward {tag} launches {counts}", sha(counts.encode()))
        del ws

    grads = {}
    for dim, fp32, B, H, W in TRAIN:
        da = dim | (FP32 if fp32 else 0)
        p, pk, pkb = net(dim, "he")
        x = (hash_randn((B, 3, H, W), 800 + W) * 0.9).to(dev)
        gy = (hash_randn((B, 3, H, W), 801 + W) * 0.1).to(dev)
        t = torch.tensor([(53 * (i + 3)) % 1000 for i in range(B)], dtype=torch.long, device=dev)
        ws = torch.empty(lib.sinddm_train_workspace_bytes(da, B, H, W), dtype=torch.uint8, device=dev)
        y, gx, gp = torch.empty(B, 3, H, W, device=dev), torch.empty(B, 3, H, W, device=dev), torch.zeros_like(p)
        _lib.check(lib.sinddm_prof_begin(), "prof_begin")
        _lib.check(lib.sinddm_net_forward_train(_lib.ptr(p), _lib.ptr(pk), _lib.ptr(x), _lib.ptr(t), 0, 2.0, _lib.ptr(y), da, B, H, W,
                                                ws.data_ptr(), ws.numel(), st), "sinddm_net_forward_train")
        _lib.check(lib.sinddm_net_backward(_lib.ptr(p), _lib.ptr(pk), _lib.ptr(pkb), _lib.ptr(x), _lib.ptr(gy), _lib.ptr(gp),
                                           _lib.ptr(gx), da, B, H, W, ws.data_ptr(), ws.numel(), st), "sinddm_net_backward")
        torch.cuda.synchronize()
        counts = launches()
        if not bool(torch.isfinite(y).all() and torch.isfinite(gx).all() and torch.isfinite(gp).all()):
            raise SystemExit("non-finite result")
        tag = f"dim{dim} fp32_convs{fp32} {B}x{H}x{W}"
        emit(f"train {tag} y", sha_t(y))
        emit(f"train {tag} grad_x", sha_t(gx))
        emit(f"train {tag} launches {counts}", sha(counts.encode()))
        grads[tag] = gp.cpu()
        del ws
    if args.grads:
        torch.save(grads, args.grads)
    finish()


if __name__ == "__main__":
    main()
