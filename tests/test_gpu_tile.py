"""Tileable sampling on the GPU: wrap-around borders per axis in the sampler chain.

No convolution kernel knows circular padding: a wrapped axis carries a halo of SINDDM_TILE_HALO = 16 wrapped pixels (the
network's receptive radius), the zero-padded kernels run on the extended image and the centre is kept
(tests/test_tile_host.py proves the construction on the CPU).  Here:

  1. sinddm_wrap_halo against F.pad(mode='circular') / modulo indexing, bit for bit, with and without `src`;
  2. sinddm_upsample_bilinear_wrap: flags (0,0) are the plain entry; wrapped axes against torch and a float64 restatement;
  3. one network evaluation through the tiled `_eps` against the circularly padded oracle;
  4. sinddm_sample_chain_tile against the oracle's chain under circular padding (caller-supplied noise);
  5. the tiled chain commutes with toroidal shifts, the plain chain does not;
  6. bit equalities: halo (0,0) = sinddm_sample_chain_ex; with / without a second stream; run to run;
  7. the tiled chain against the tiled step-by-step route over a whole scale;
  8. the public drivers return samples of the un-extended sizes.
The reference has no line for this: it would set padding_mode='circular' on its nn.Conv2d's.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from conftest import max_abs, rel_l2
from oracle import sinddm_oracle as O
from sinddm_amd.configs import CONFIGS, build_diffusion
from sinddm_amd.synth import closed_form_state_dict, closed_form_tensor, hash_randn, he_state_dict, noise_key
from tile_util import HALO, centre, circular_oracle, wrap_pad

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -777.0

_DIFF = {}


def _he_state_dict(dim):
    """sinddm_amd.synth.he_state_dict(dim), built once per module.  (At dim 160 the closed-form fill gives an output that is
    almost constant over the image -- rms 0.27, spatial std 0.001 --, so whatever its borders do vanishes in a whole-tensor
    norm: on the CPU oracle one zero-padded evaluation is 1.9e-3 from shift-equivariant and a plain 4-step chain 1.5e-5 from
    the circular one, below the chain budget.  With He weights the oracle's plain chain is 0.21 from equivariant, one
    evaluation 0.36: the chain tests can tell the paddings apart.)"""
    if dim not in _HE:
        _HE[dim] = he_state_dict(dim)
    return _HE[dim]


_HE = {}


def _diff(dim, cfg="C2", weights="closed_form"):
    """(net, diffusion) of a config, built once per module; tests set `tile` / hooks and must put them back."""
    if (dim, cfg, weights) not in _DIFF:
        _DIFF[(dim, cfg, weights)] = build_diffusion(cfg, dim=dim, device=DEV)
        if weights == "he":
            _DIFF[(dim, cfg, weights)][0].load_state_dict(_he_state_dict(dim))
    net, d = _DIFF[(dim, cfg, weights)]
    d.tile, d.noise_fn, d.chain_noise, d.two_streams, d.img_prev_upsample = (False, False), None, False, True, None
    return net, d


def _fill(n, seed, stream):
    from sinddm_amd import _lib
    lib = _lib.load()
    out = torch.empty(n, device=DEV)
    _lib.check(lib.sinddm_normal_fill(_lib.ptr(out), n, seed, stream, _lib.stream_ptr(DEV)), "sinddm_normal_fill")
    return out


# ---- 1: sinddm_wrap_halo ---------------------------------------------------------------------------------------------------
# (BC, H, W, halo_y, halo_x, guard floats in front of ext).  17x19 and 5x7 take the one-float kernel (W % 4 != 0); 12x16 with
# an aligned base takes the 16-byte kernel, with a base 3 floats off the one-float kernel again.
HALO_CASES = [(6, 17, 19, 16, 16, 8), (6, 17, 19, 0, 16, 8), (6, 17, 19, 16, 0, 8), (6, 5, 7, 16, 16, 8),
              (6, 12, 16, 16, 16, 8), (6, 12, 16, 16, 16, 3), (6, 12, 16, 16, 0, 8), (6, 12, 16, 0, 20, 8)]


@pytest.mark.parametrize("BC,H,W,hy,hx,guard", HALO_CASES, ids=lambda v: str(v))
def test_wrap_halo_bit_for_bit(BC, H, W, hy, hx, guard):
    from sinddm_amd import _lib
    lib = _lib.load()
    src = hash_randn((BC, H, W), 3 + H).to(DEV)
    expect = wrap_pad(src, hy, hx)                                      # modulo indexing: also wraps more than once (5x7)
    if hy <= H and hx <= W:
        assert torch.equal(expect, F.pad(src[None], (hx, hx, hy, hy), mode="circular")[0])
    He, We = H + 2 * hy, W + 2 * hx
    n = BC * He * We
    for in_place in (False, True):
        big = torch.full((guard + n + 8,), SENTINEL, device=DEV)
        ext = big[guard:guard + n].view(BC, He, We)
        if in_place:                                                    # a valid centre inside a halo of other numbers
            ext.fill_(5.0)
            ext[:, hy:hy + H, hx:hx + W] = src
        rc = lib.sinddm_wrap_halo(big.data_ptr() + 4 * guard, None if in_place else _lib.ptr(src), BC, H, W, hy, hx,
                                  _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(ext, expect), ("in place" if in_place else "src")
        assert bool((big[:guard] == SENTINEL).all()) and bool((big[guard + n:] == SENTINEL).all())
    # the Python helper is this call
    from sinddm_amd.models import MultiScaleGaussianDiffusion
    assert torch.equal(MultiScaleGaussianDiffusion._wrap_pad(src.view(2, 3, H, W), hy, hx), expect.view(2, 3, He, We))


# ---- 2: sinddm_upsample_bilinear_wrap ----------------------------------------------------------------------------------------
def _up(x, size, flags=None):
    from sinddm_amd import _lib
    lib = _lib.load()
    B, Cc, h, w = x.shape
    out = torch.empty((B, Cc) + tuple(size), device=DEV)
    if flags is None:
        rc = lib.sinddm_upsample_bilinear(_lib.ptr(x), _lib.ptr(out), B * Cc, h, w, size[0], size[1], _lib.stream_ptr(DEV))
    else:
        rc = lib.sinddm_upsample_bilinear_wrap(_lib.ptr(x), _lib.ptr(out), B * Cc, h, w, size[0], size[1], flags[0], flags[1],
                                               _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0
    return out


def _up_f64(x, size, flags):
    """Bilinear interpolation (align_corners=False) in float64; on a wrapped axis of the periodic continuation of x."""
    x = x.double()

    def axis(n_in, n_out, wrap):
        f = (n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
        if wrap:
            i0 = np.floor(f)
            lam = f - i0
            i0 = i0.astype(np.int64) % n_in
            i1 = (i0 + 1) % n_in
        else:
            f = np.maximum(f, 0.0)
            i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
            i1 = np.minimum(i0 + 1, n_in - 1)
            lam = f - i0
        return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(lam)

    y0, y1, ly = axis(x.shape[2], size[0], flags[0])
    x0, x1, lx = axis(x.shape[3], size[1], flags[1])
    ly, lx = ly[None, None, :, None], lx[None, None, None, :]
    top, bot = x[:, :, y0, :], x[:, :, y1, :]
    return (1 - ly) * ((1 - lx) * top[..., x0] + lx * top[..., x1]) + ly * ((1 - lx) * bot[..., x0] + lx * bot[..., x1])


def test_upsample_wrap():
    """The bound is test_upsample_golden's (max-abs 2e-5)."""
    x = closed_form_tensor((2, 3, 48, 64), phase=0.9, amp=1.0, freq=0.271).to(DEV)
    assert torch.equal(_up(x, (67, 90), (0, 0)), _up(x, (67, 90)))
    small = closed_form_tensor((2, 3, 12, 16), phase=0.4, amp=1.0, freq=0.271)
    ref = F.interpolate(F.pad(small, (2, 2, 2, 2), mode="circular"), scale_factor=2, mode="bilinear")[:, :, 4:-4, 4:-4]
    got = _up(small.to(DEV), (24, 32), (1, 1)).cpu()
    assert ref.shape == got.shape
    print(f"upsample wrap (1, 1) 12x16 -> 24x32 vs torch on the circularly padded source: max-abs {max_abs(got, ref):.2e}")
    assert max_abs(got, ref) <= 2e-5
    assert max_abs(_up(small.to(DEV), (24, 32)).cpu(), ref) > 1e-2         # the plain entry clamps at the border
    for flags in ((1, 1), (0, 1)):
        got = _up(x, (67, 90), flags).cpu()
        err = max_abs(got, _up_f64(x.cpu(), (67, 90), flags))
        print(f"upsample wrap {flags} 48x64 -> 67x90 vs float64: max-abs {err:.2e}")
        assert err <= 2e-5
    assert max_abs(_up(x, (67, 90)).cpu(), _up_f64(x.cpu(), (67, 90), (0, 0))) <= 2e-5     # (the restatement itself)
    # MultiScaleGaussianDiffusion.upsample takes the wrap variant when `tile` is set
    net, d = _diff(32)
    d.tile = (False, True)
    assert torch.equal(d.upsample(x, (67, 90)), _up(x, (67, 90), (0, 1)))
    d.tile = (False, False)
    assert torch.equal(d.upsample(x, (67, 90)), _up(x, (67, 90)))


# ---- 3: one network evaluation through the tiled _eps -------------------------------------------------------------------------
@pytest.mark.parametrize("dim,B,H,W,tile", [(32, 2, 17, 19, (True, True)), (160, 2, 48, 64, (True, True)),
                                            (160, 2, 67, 90, (False, True))], ids=["dim32_17x19_xy", "dim160_48x64_xy", "dim160_67x90_x"])
def test_tiled_eps_vs_circular_oracle(dim, B, H, W, tile):
    """rel-L2 < 1e-5: the bound of test_net_forward_vs_oracle_edges for the same comparison without tiling."""
    net, d = _diff(dim)
    sd = closed_form_state_dict(dim)
    x = hash_randn((B, 3, H, W), 11 + H)
    t = 9
    with torch.no_grad(), circular_oracle(tile):
        ref = O.net_forward(sd, x, torch.full((B,), t, dtype=torch.long), 1)
    plain = d._eps(x.to(DEV), None, t, 1)
    d.tile = tile
    got = d._eps(x.to(DEV), None, t, 1)
    d.tile = (False, False)
    assert got.shape == x.shape and got.is_contiguous()
    err = rel_l2(got.cpu(), ref)
    print(f"dim {dim} B={B} {H}x{W} tile={tile}: tiled eps vs circular oracle rel-L2 {err:.2e}; "
          f"untiled eps vs circular oracle {rel_l2(plain.cpu(), ref):.2e}")
    assert err < 1e-5
    # teeth: without the halo the same call misses the bound tenfold (the closed-form weights give an almost constant eps at
    # dim 160 -- spatial std 0.001 of an rms of 0.27 --, so the borders weigh little in a whole-tensor norm: 4e-4 .. 1.4e-3)
    assert rel_l2(plain.cpu(), ref) > 1e-4


# ---- the library call ----------------------------------------------------------------------------------------------------------
def _chain_tile(net, d, s, x_ext, xt_ext, ts, dim, hy, hx, seed=0, aux=False, noise=None, entry="tile"):
    """sinddm_sample_chain_tile (or _ex) on extended buffers; returns the whole extended result."""
    from sinddm_amd import _lib
    from sinddm_amd.models import _aux_stream, _workspace
    lib = _lib.load()
    B, _, He, We = x_ext.shape
    n = len(ts)
    xa, xb, eps = x_ext.clone(), torch.empty_like(x_ext), torch.empty_like(x_ext)
    tab = d._coef_table(s)
    coefs = (_lib.StepCoefs * n)(*[tab[t] for t in ts])
    tl = (C.c_int * n)(*ts)
    ws = _workspace(DEV, lib.sinddm_workspace_bytes(dim, B, He, We))
    flag = C.c_int(-1)
    opts = _lib.ChainOpts()
    opts.noise = _lib.ptr(noise)
    args = [_lib.ptr(net.flat_params), _lib.ptr(net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt_ext),
            coefs, tl, n, float(s), seed, 0, dim]
    tail = [ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV), _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts)]
    if entry == "tile":
        rc = lib.sinddm_sample_chain_tile(*args, B, He - 2 * hy, We - 2 * hx, *tail, hy, hx)
    else:
        assert hy == 0 and hx == 0
        rc = lib.sinddm_sample_chain_ex(*args, B, He, We, *tail)
    torch.cuda.synchronize()
    assert rc == 0 and flag.value in (0, 1)
    return xb if flag.value == 1 else xa


def _inputs(B, H, W, n_steps, key):
    x0 = hash_randn((B, 3, H, W), key) * 0.8
    xt = (hash_randn((B, 3, H, W), key + 1) * 0.5).clamp(-1, 1)
    z = torch.stack([hash_randn((B, 3, H, W), key + 2 + i) for i in range(n_steps)])
    return x0, xt, z


def _ext(t, hy, hx, halo_value=None):
    """The wrapped extension on the device; `halo_value`: that number in the halo instead (for buffers whose halo the call
    must not depend on)."""
    e = wrap_pad(t, hy, hx)
    if halo_value is not None:
        H, W = t.shape[-2], t.shape[-1]
        c = e[..., hy:hy + H, hx:hx + W].clone()
        e.fill_(halo_value)
        e[..., hy:hy + H, hx:hx + W] = c
    return e.to(DEV).contiguous()


# (scale, steps): scale 0 runs mode 0 (its t = 0 step adds no noise); scale 1 runs modes 1, 1, 1 and, at t = 0, 2
RUNS = {0: [700, 300, 1, 0], 1: [300, 200, 100, 0]}


# ---- 4: the chain against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1], ids=["scale0", "scale1"])
@pytest.mark.parametrize("dim,B,H,W", [(32, 2, 24, 40), (160, 16, 67, 90)], ids=["dim32_B2_24x40", "dim160_B16_67x90"])
def test_tiled_chain_vs_circular_oracle(dim, B, H, W, s):
    """4 steps with caller-supplied noise from a fixed start, replayed with oracle.p_sample under circular padding on the
    same centre noise: rel-L2 <= 1e-4, the project's chain budget.  He-normal weights (`_he_state_dict`): with the
    closed-form fill the zero-padded chain itself sits 1.5e-5 from the circular oracle.  The halo of the start and of the noise slots holds
    other numbers: the call refreshes the first and never uses the second.  (dim 160, B = 16: the extended 99x122 takes
    the padded-row tail kernel and two streams.)"""
    net, d = _diff(dim, weights="he")
    cfg = CONFIGS["C2"]
    sched = O.make_schedule(cfg["T"], len(cfg["sizes"]), cfg["rescale_losses"], 1, train_full_t=True)
    sd = _he_state_dict(dim)
    ts = RUNS[s]
    x0, xt, z = _inputs(B, H, W, len(ts), 40 + s)
    ref = x0
    with torch.no_grad(), circular_oracle((True, True)):
        for i, t in enumerate(ts):
            ref = O.p_sample(sched, sd, ref, t, s, z[i], xt if s > 0 else None)
    out = _chain_tile(net, d, s, _ext(x0, HALO, HALO, 3.0), _ext(xt, HALO, HALO) if s > 0 else None, ts, dim, HALO, HALO,
                      aux=True, noise=_ext(z, HALO, HALO, 50.0))
    assert torch.isfinite(out).all()
    got = centre(out, HALO, HALO)
    assert torch.equal(out, wrap_pad(got, HALO, HALO))                  # the result's halo is its wrapped centre
    err = rel_l2(got.cpu(), ref)
    plain = _chain_tile(net, d, s, x0.to(DEV), xt.to(DEV) if s > 0 else None, ts, dim, 0, 0, aux=True, noise=z.to(DEV), entry="ex")
    far = rel_l2(plain.cpu(), ref)
    print(f"dim {dim} B={B} {H}x{W} s={s} ts={ts}: tiled chain vs circular oracle rel-L2 {err:.2e}; "
          f"the zero-padded chain vs circular oracle {far:.2e}")
    assert err <= 1e-4
    assert far > 1e-2                                                   # the comparison tells the two paddings apart


# ---- 5: toroidal shifts ----------------------------------------------------------------------------------------------------------
def test_tiled_chain_commutes_with_toroidal_shifts():
    """dim 160, B = 16, 67x90, scale 1, 4 steps: start, x-tilde and noise centres rolled by (5, 7) and re-padded.  The chain
    of the circular network is exactly equivariant and both tiled runs sit within 1e-4 of it: 2e-4 by the triangle
    inequality.  The plain chain (zero padding) must differ by more than 1e-2.

    Weights: He-normal from the hash generator (`_he_state_dict`): with the closed-form fill this experiment measured 1.7e-5
    for the plain chain on the GPU -- it could not tell the two paddings apart.  The 1e-4 premise is checked here once
    more: the first and the last chain of the tiled run (one of each half-batch) against oracle.p_sample under circular
    padding."""
    dim, B, H, W, s = 160, 16, 67, 90, 1
    net, d = _diff(dim, weights="he")
    ts = RUNS[s]
    x0, xt, z = _inputs(B, H, W, len(ts), 40 + s)
    roll = lambda t: torch.roll(t, (5, 7), (-2, -1))
    a = centre(_chain_tile(net, d, s, _ext(x0, HALO, HALO), _ext(xt, HALO, HALO), ts, dim, HALO, HALO, aux=True,
                           noise=_ext(z, HALO, HALO)), HALO, HALO)
    b = centre(_chain_tile(net, d, s, _ext(roll(x0), HALO, HALO), _ext(roll(xt), HALO, HALO), ts, dim, HALO, HALO, aux=True,
                           noise=_ext(roll(z), HALO, HALO)), HALO, HALO)
    err = rel_l2(b.cpu(), roll(a.cpu()))
    pa = _chain_tile(net, d, s, x0.to(DEV), xt.to(DEV), ts, dim, 0, 0, aux=True, noise=z.to(DEV), entry="ex")
    pb = _chain_tile(net, d, s, roll(x0).to(DEV), roll(xt).to(DEV), ts, dim, 0, 0, aux=True, noise=roll(z).to(DEV), entry="ex")
    far = rel_l2(pb.cpu(), roll(pa.cpu()))
    cfg = CONFIGS["C2"]
    sched = O.make_schedule(cfg["T"], len(cfg["sizes"]), cfg["rescale_losses"], 1, train_full_t=True)
    sd, idx = _he_state_dict(dim), [0, B - 1]
    ref = x0[idx]
    with torch.no_grad(), circular_oracle((True, True)):
        for i, t in enumerate(ts):
            ref = O.p_sample(sched, sd, ref, t, s, z[i][idx], xt[idx])
    to_oracle = rel_l2(a[idx].cpu(), ref)
    print(f"toroidal shift (5,7): tiled chain rel-L2 {err:.2e}; plain chain {far:.2e}; tiled chain vs circular oracle "
          f"(chains 0 and {B - 1}) {to_oracle:.2e}")
    assert to_oracle <= 1e-4
    assert err <= 2e-4
    assert far > 1e-2


# ---- 6: bit equalities -------------------------------------------------------------------------------------------------------------
def test_tiled_chain_bit_equalities():
    dim, B = 160, 16
    net, d = _diff(dim)
    for s, (H, W) in ((0, (48, 64)), (1, (67, 90))):
        ts = RUNS[s]
        x0, xt, _ = _inputs(B, H, W, 1, 60 + s)
        xd, td = x0.to(DEV), (xt.to(DEV) if s > 0 else None)
        # halo (0, 0) is sinddm_sample_chain_ex: Philox noise, one seed
        for aux in (False, True):
            y_ex = _chain_tile(net, d, s, xd, td, ts, dim, 0, 0, seed=9091, aux=aux, entry="ex")
            y_t0 = _chain_tile(net, d, s, xd, td, ts, dim, 0, 0, seed=9091, aux=aux)
            assert torch.equal(y_ex, y_t0), (s, aux)
    # tiled: with and without the second stream, and run to run
    xe, te = _ext(x0, HALO, HALO), _ext(xt, HALO, HALO)
    y1 = _chain_tile(net, d, 1, xe, te, ts, dim, HALO, HALO, seed=77, aux=True)
    y2 = _chain_tile(net, d, 1, xe, te, ts, dim, HALO, HALO, seed=77, aux=False)
    y3 = _chain_tile(net, d, 1, xe, te, ts, dim, HALO, HALO, seed=77, aux=True)
    assert torch.equal(y1, y2) and torch.equal(y1, y3)
    assert torch.equal(y1, wrap_pad(centre(y1, HALO, HALO), HALO, HALO))
    # per axis: a halo on x only
    xe, te = _ext(x0, 0, HALO), _ext(xt, 0, HALO)
    y4 = _chain_tile(net, d, 1, xe, te, ts, dim, 0, HALO, seed=77, aux=True)
    assert torch.equal(y4, _chain_tile(net, d, 1, xe, te, ts, dim, 0, HALO, seed=77, aux=False))
    assert torch.equal(y4, wrap_pad(centre(y4, 0, HALO), 0, HALO)) and torch.isfinite(y4).all()


# ---- 7: chain against the step-by-step route over a whole scale ------------------------------------------------------------------
def test_tiled_chain_noise_equals_tiled_stepwise_over_a_scale(golden):
    """`tile = (True, True)` with a keyed `noise_fn` over the whole scale 1 of C1 (T = 100, 67x90, B = 2, dim 32; the input
    is the pyramid's coarsest image, upsampled): `chain_noise = True` (sinddm_sample_chain_tile) against the step-by-step
    route (`_eps` pads, evaluates and crops; the step kernel runs on the centre).  The bound is the one
    test_gpu_chain_guided.py applies to its own chain_noise-against-stepwise comparison: 2 x 0.0, bit for bit -- both routes
    launch the same network kernels on the same extended input, and the fused tail evaluates the step as the separate
    kernels do."""
    net, d = _diff(32, "C1")
    s, B = 1, 2
    pyr = golden("c1_pyramid.npz")
    img0 = torch.from_numpy(pyr["scale_0"].transpose(2, 0, 1).copy()).float().div(255).mul(2).sub(1)[None].repeat(B, 1, 1, 1)
    d.tile = (True, True)
    img = d.upsample(img0.to(DEV), d.image_sizes[s])
    assert tuple(img.shape[2:]) == (67, 90)
    fetched = []

    def keyed(kind, shape, ss, tt, dev):
        fetched.append((kind, tuple(shape), ss, tt))
        return _fill(int(np.prod(shape)), noise_key(kind, ss, tt), 0).view(shape)

    d.noise_fn = keyed
    ref = d.p_sample_via_scale_loop(B, img, s)
    order_ref, fetched[:] = list(fetched), []
    assert len(order_ref) == d.num_timesteps_ideal[s] and all(e[1] == (B, 3, 67, 90) for e in order_ref)
    d.chain_noise = True
    d.draw_log = []
    got = d.p_sample_via_scale_loop(B, img, s)
    torch.cuda.synchronize()
    d.draw_log = None
    assert fetched == order_ref
    assert got.shape == ref.shape == img.shape and torch.isfinite(got).all()
    err = max_abs(got.cpu(), ref.cpu())
    print(f"C1 s=1 67x90 B=2 {len(order_ref) - 1} steps tiled: chain_noise vs stepwise max-abs {err:.3e} "
          f"rel-L2 {rel_l2(got.cpu(), ref.cpu()):.3e}")
    assert err <= 2 * 0.0
    # the tiled run is another sample than the plain one
    d.tile = (False, False)
    plain = d.p_sample_via_scale_loop(B, img, s)
    assert rel_l2(plain.cpu(), ref.cpu()) > 1e-3
    # without a noise_fn the run logs the tiled chain call
    d.noise_fn, d.chain_noise, d.tile, d.draw_log = None, False, (True, False), []
    torch.manual_seed(5)
    d._run_steps(img, s, [3, 2, 1, 0])
    log, d.draw_log = d.draw_log, None
    assert len(log) == 1 and log[0][0] == "chain_tile" and log[0][1] == s and log[0][3] == [3, 2, 1, 0] and log[0][4] == (HALO, 0)


# ---- 8: Python end to end ------------------------------------------------------------------------------------------------------------
def _trainer(golden, tmp_path, dim=32, T=20, batch=2):                     # the C1 recipe of tests/test_gpu_e2e.py
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    from sinddm_amd.trainer import MultiscaleTrainer
    meta = golden("g11_img_scales.json")["C1"]
    pyr = golden("c1_pyramid.npz")
    folder = str(tmp_path / "balloons") + "/"
    for key in pyr.files:
        os.makedirs(folder + key, exist_ok=True)
        Image.fromarray(pyr[key]).save(folder + key + "/balloons.png")
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    net.load_state_dict(closed_form_state_dict(dim))
    sizes = [tuple(s) for s in meta["sizes"]]
    d = MultiScaleGaussianDiffusion(net, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"], image_sizes=sizes,
                                    timesteps=T, train_full_t=True, scale_losses=meta["rescale_losses"], loss_factor=1,
                                    loss_type="l1", device=DEV, reblurring=True, omega=0,
                                    results_folder=str(tmp_path / "res")).to(DEV)
    tr = MultiscaleTrainer(d, folder=folder, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"],
                           image_sizes=sizes, train_batch_size=batch, train_lr=1e-3, train_num_steps=6,
                           gradient_accumulate_every=1, step_start_ema=2, update_ema_every=2,
                           save_and_sample_every=10 ** 9, avg_window=2, sched_milestones=[3],
                           results_folder=str(tmp_path / "res"), device=DEV)
    return tr, meta


def test_public_drivers_with_tile(golden, tmp_path):
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    sizes = [tuple(s) for s in meta["image_sizes_hw"]]
    em.tile = (False, True)
    em.draw_log = []
    torch.manual_seed(99)
    outs = tr.sample_scales(batch_size=2, custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    log, em.draw_log = em.draw_log, None
    assert [tuple(o.shape) for o in outs] == [(2, 3) + hw for hw in sizes]
    assert all(torch.isfinite(o).all() for o in outs)
    assert [e[0] for e in log] == ["init", "chain_tile", "renoise", "chain_tile", "renoise", "chain_tile"]
    assert all(e[4] == (0, HALO) for e in log if e[0] == "chain_tile")
    em.tile = (True, True)
    outs = tr.roi_guided_sampling(custom_t_list=em.num_timesteps_ideal[1:], target_roi=[10, 12, 30, 40],
                                  roi_bb_list=[[20, 30, 40, 36], [35, 50, 30, 30]], save_unbatched=False, batch_size=2,
                                  scale_mul=(1, 1), save_images=False)
    assert [tuple(o.shape) for o in outs] == [(2, 3) + hw for hw in sizes]
    assert all(torch.isfinite(o).all() for o in outs)
    # the edit maps were padded consistently: the guided tiled run is the step-by-step guided tiled run on the same draws
    em.roi_guided_sampling, em.roi_bbs = True, [[20, 30, 40, 36], [35, 50, 30, 30]]
    H, W = sizes[0]
    x0 = (hash_randn((2, 3, H, W), 8) * 0.8).to(DEV)
    em.noise_fn = lambda kind, shape, ss, tt, dev: _fill(int(np.prod(shape)), noise_key(kind, ss, tt), 0).view(shape)
    try:
        em.chain_noise = True
        a = em._run_steps(x0, 0, [19, 10, 0])
        em.chain_noise = False
        b = em._run_steps(x0, 0, [19, 10, 0])
        em.roi_guided_sampling = False
        c = em._run_steps(x0, 0, [19, 10, 0])
    finally:
        em.roi_guided_sampling, em.noise_fn = False, None
    assert max_abs(a.cpu(), b.cpu()) <= 4e-6 * max(1.0, float(b.abs().max()))       # the bound of test_fused_edit_equals_stepwise_edit
    assert max_abs(a.cpu(), c.cpu()) > 1e-2                                         # the edit is not a no-op
