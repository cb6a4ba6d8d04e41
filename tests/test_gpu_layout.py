"""Layout conditioning inside the fused sampler chain (sinddm_sample_chain_layout, sinddm_layout_delta,
sinddm_reverse_step_layout; `layout_maps`, `paint2image`): at every conditioned reverse step the low spatial frequencies of
the predicted clean image are pulled to those of a layout picture.

The reference has no counterpart, so the yardsticks are the float64 restatement of the contract (tests/layout_util.py), the
project's own step-by-step route and exactness properties:
  3. sinddm_layout_delta against the restatement, bound derived from the fp32 reduction;
  4. sinddm_reverse_step_layout against the restatement fed the kernel's own D, modes 0 / 1 / 2, keep and edit off and on;
  5. N = 1 against sinddm_reverse_step_edit with ew = 1 - g, ec = g L;
  6. one full-strength pull contracts the low band of the residual on the device as it does on paper;
  7. the fused chain equals the same walk step by step on every tail kernel's shape and tiled; `_run_steps` is that call;
  8. bit-level identities: the option off is sinddm_sample_chain_resample; one / two streams; re-run; Philox / buffers;
  9. a seeded sample at batch 1, position 2 of 3 and position 12 of 16;
 10. every SINDDM_E_BADARG of the new entry, none of which touches the device;
 11. `paint2image` on the C1 pyramid.
Shapes: the four of test_gpu_chain_guided.SHAPES (one tail kernel each; three steps incl. t = 0) and the tiled case of
test_gpu_keep.CASES.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import layout_util as LU
from conftest import max_abs, rel_l2
from sinddm_amd.synth import hash_randn
from test_gpu_chain_guided import _trainer
from test_gpu_keep import CASE_IDS, CASES, _bound, _Ctx, _draw, _known
from test_gpu_seeds import BUDGET, _ctx, _dev_seeds, _sample_draws, _seed_list

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_CHAIN = 8                                                  # the block size of the chain tests
G_CHAIN = (1.0, 1.0, 0.0)                                    # ... and their strengths: the last step stays fused


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _cells(H, W, N):
    return -(-H // N), -(-W // N)


def _layout(H, W, key=83):
    return _known(H, W, key)                                 # (3, H, W) in [-1, 1], unrelated to every sample


def _chain_lay(c, x0, ts, seed=0, sid0=0, aux=False, edit=None, keep=None, noise=None, seeds=None, lay=None, g=G_CHAIN,
               N=N_CHAIN, lo="on", entry="layout"):
    """sinddm_sample_chain_layout (or _resample) on centre-size arguments of a test_gpu_keep._Ctx, extended here.  `lo`: 'on'
    (layout + g), 'null' (no option block), 'no_layout' (a block whose layout is NULL).  Returns the extended result; the
    delta scratch is left in `c.last_delta`."""
    from sinddm_amd import _lib
    from sinddm_amd.models import _aux_stream, _workspace
    lib = _lib.load()
    xa = c.ext(x0).clone()
    B, _, H, We = xa.shape
    n = len(ts)
    xb, eps, xt = torch.empty_like(xa), torch.empty_like(xa), c.ext(c.xt)
    tab = c.d._coef_table(c.s)
    coefs = (_lib.StepCoefs * n)(*[tab[t] for t in ts])
    tl = (C.c_int * n)(*ts)
    ws = _workspace(DEV, lib.sinddm_workspace_bytes(c.dim, B, H, We))
    flag = C.c_int(-1)
    opts = _lib.ChainOpts()
    held = []
    if edit is not None:
        held += [c.ext(edit[0]), c.ext(edit[1])]
        opts.edit_w, opts.edit_c = _lib.ptr(held[0]), _lib.ptr(held[1])
    opts.noise = _lib.ptr(noise)
    kopts = None
    if keep is not None:
        held += [c.ext(keep[0]), c.ext(keep[1])]
        ab_tab = c.d._keep_ab_table()
        ab = (C.c_float * (2 * n))(*[float(v) for t in ts for v in ab_tab[t]])
        kopts = _lib.KeepOpts()
        kopts.mask, kopts.x0, kopts.ab = _lib.ptr(held[-2]), _lib.ptr(held[-1]), C.cast(ab, C.POINTER(C.c_float))
    sd = _dev_seeds(seeds) if seeds is not None else None
    args = [_lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
            coefs, tl, n, float(c.s), seed, sid0, c.dim, B, H, We - 2 * c.hx, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
            _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, c.hx,
            C.byref(kopts) if kopts is not None else None, _lib.ptr(sd), None]
    if entry == "resample":
        rc = lib.sinddm_sample_chain_resample(*args)
    else:
        lopts = _lib.LayoutOpts()
        h, w = _cells(H, We - 2 * c.hx, N)
        c.last_delta = torch.full((B, 3, h, w), 7.5, device=DEV)
        garr = (C.c_float * n)(*[float(v) for v in g[:n]])
        if lo != "no_layout":
            held.append(c.ext(lay))
            lopts.layout = _lib.ptr(held[-1])
        lopts.down, lopts.g, lopts.delta = N, C.cast(garr, C.POINTER(C.c_float)), _lib.ptr(c.last_delta)
        rc = lib.sinddm_sample_chain_layout(*args, None if lo == "null" else C.byref(lopts))
    torch.cuda.synchronize()
    assert rc == 0 and flag.value in (0, 1)
    return xb if flag.value == 1 else xa


def _delta(k, L, x, eps, xt, ew, ec, N, halo=(0, 0)):
    """sinddm_layout_delta on buffer-size tensors; (B, 3, h, w)."""
    from sinddm_amd import _lib
    lib = _lib.load()
    B, _, H, W = x.shape
    Hc, Wc = H - 2 * halo[0], W - 2 * halo[1]
    D = torch.full((B, 3) + _cells(Hc, Wc, N), 7.5, device=DEV)
    rc = lib.sinddm_layout_delta(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(L), _lib.ptr(D), C.byref(k), _lib.ptr(ew),
                                 _lib.ptr(ec), N, B, Hc, Wc, halo[0], halo[1], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0
    return D


def _step(k, x, eps, xt, z, D, g, N, ew=None, ec=None, km=None, kx=None, ka=1.0, kb=0.0, wrap=(0, 0)):
    from sinddm_amd import _lib
    lib = _lib.load()
    B, _, H, W = x.shape
    out = torch.empty_like(x)
    rc = lib.sinddm_reverse_step_layout(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(out), C.byref(k),
                                        _lib.ptr(D), g, N, _lib.ptr(ew), _lib.ptr(ec), _lib.ptr(km), _lib.ptr(kx), ka, kb, B, H, W,
                                        0, 0, wrap[0], wrap[1], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def diff20():
    from sinddm_amd.configs import build_diffusion
    return build_diffusion("C2", dim=20, device=DEV)[1]


def _inputs(B, H, W, key=50):
    x, eps, xt, z = ((hash_randn((B, 3, H, W), key + i) * a).to(DEV) for i, a in enumerate((0.8, 1.0, 0.5, 1.0)))
    ew = (0.2 + 0.8 * hash_randn((H, W), key + 10).abs().clamp(0, 1)).to(DEV)
    ec = (hash_randn((3, H, W), key + 11) * 0.3).to(DEV)
    return x, eps, xt, z, ew, ec


def _delta_bound(k, L, x, eps, xt, ew, ec, N):
    """(n_blk + 8) 2^-24 A: every term of the mean carries fewer than 8 roundings, an fp32 mean of n terms adds at most
    n - 1 more; A bounds a term's magnitude through the magnitudes of what it is made of."""
    H, W = x.shape[-2:]
    n_blk = min(N, H) * min(N, W)
    gam = float(k.gamma_t) if k.mode != 0 else 0.0
    A = L.abs()[None] + (ew.abs() if ew is not None else 1.0) * (
        k.sqrt_recip_ac_t * x.abs() + k.sqrt_recipm1_ac_t * eps.abs() + gam * xt.abs()) / (1.0 - gam)
    if ec is not None:
        A = A + ec.abs()[None]
    return (n_blk + 8) * 2.0 ** -24 * float(A.max())


# ---- 3: the block delta ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,t", [(0, 700), (1, 400)], ids=["mode0", "mode1"])
@pytest.mark.parametrize("H,W,N", [(33, 50, 8), (25, 34, 16), (48, 64, 4), (67, 90, 3), (7, 9, 16)])
def test_layout_delta_against_float64(diff20, H, W, N, s, t):
    k = diff20.step_coefs(t, s)
    assert k.mode == s
    x, eps, xt, _, ew, ec = _inputs(3, H, W)
    L = _layout(H, W)
    for edit in (False, True):
        e = (ew, ec) if edit else (None, None)
        D = _delta(k, L, x, eps, xt, *e, N)
        ref = LU.delta(k, _np(L), _np(x), _np(eps), _np(xt), _np(e[0]), _np(e[1]), N)
        err, bound = float(np.abs(_np(D) - ref).max()), _delta_bound(k, L, x, eps, xt, *e, N)
        print(f"layout_delta {H}x{W} N={N} mode {k.mode} edit={edit}: max-abs vs float64 {err:.3e} (bound {bound:.3e}, "
              f"max|D| {np.abs(ref).max():.3f})")
        assert D.shape == ref.shape and err <= bound


# ---- 4: the conditioned step -------------------------------------------------------------------------------------------------
# (mode 0 at t = 10: the pull reaches the output through coef1_t, 0.125 there and 0.0035 at t = 700)
MODES = [(0, 10), (1, 400), (1, 0)]
MODE_IDS = ["mode0", "mode1", "mode2"]


@pytest.mark.parametrize("s,t", MODES, ids=MODE_IDS)
def test_reverse_step_layout_against_float64(diff20, s, t):
    d = diff20
    k = d.step_coefs(t, s)
    assert k.mode == MODES.index((s, t))
    for (H, W), N, g in (((5, 7), 2, 1.0), ((5, 7), 3, 0.7), ((8, 12), 2, 0.7), ((8, 12), 3, 1.0)):
        x, eps, xt, z, ew, ec = _inputs(2, H, W, key=150)
        L, m, k0 = _layout(H, W), (hash_randn((H, W), 160) > 0).float().to(DEV), _known(H, W, 71)
        m[0, 0], m[-1, -1] = 0.25, 0.0
        for edit in (False, True):
            e = (ew, ec) if edit else (None, None)
            D = _delta(k, L, x, eps, xt, *e, N)
            for keep in (False, True):
                ka, kb = (0.8, 0.6) if keep else (1.0, 0.0)
                out = _step(k, x, eps, xt, z, D, g, N, *e, *((m, k0) if keep else (None, None)), ka, kb)
                ref = LU.layout_step(k, _np(x), _np(eps), _np(xt), _np(z), _np(D), g, N, _np(e[0]), _np(e[1]),
                                     (_np(m), _np(k0), ka, kb) if keep else None)
                err, bound = float(np.abs(_np(out) - ref).max()), 4e-6 * max(1.0, float(np.abs(ref).max()))
                print(f"reverse_step_layout {H}x{W} N={N} g={g} mode {k.mode} edit={edit} keep={keep}: max-abs vs float64 "
                      f"{err:.3e} (bound {bound:.3e})")
                assert err <= bound
                # the same step with the x axis wrapped (the halo-less flag of the step-by-step route): U differs at the borders
                out_w = _step(k, x, eps, xt, z, D, g, N, *e, *((m, k0) if keep else (None, None)), ka, kb, wrap=(0, 1))
                ref_w = LU.layout_step(k, _np(x), _np(eps), _np(xt), _np(z), _np(D), g, N, _np(e[0]), _np(e[1]),
                                       (_np(m), _np(k0), ka, kb) if keep else None, wrap=(False, True))
                err_w = float(np.abs(_np(out_w) - ref_w).max())
                print(f"    ... x axis wrapped: {err_w:.3e} (bound {4e-6 * max(1.0, float(np.abs(ref_w).max())):.3e})")
                assert err_w <= 4e-6 * max(1.0, float(np.abs(ref_w).max()))
                if not keep:
                    assert float(np.abs(ref_w - ref).max()) > 1e-3              # (the wrap is not a no-op)
                if g == 1.0 and not edit and not keep:        # (the pull is not a no-op)
                    plain = LU.step(k, _np(x), _np(eps), _np(xt), _np(z), 1.0, 0.0)
                    assert float(np.abs(ref - plain).max()) > 1e-2


# ---- 5: N = 1 is an ROI edit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,t", MODES, ids=MODE_IDS)
def test_block_one_equals_the_roi_edit(diff20, s, t):
    from sinddm_amd import _lib
    lib = _lib.load()
    k = diff20.step_coefs(t, s)
    B, H, W, g = 2, 37, 45, 0.6
    x, eps, xt, z, _, _ = _inputs(B, H, W, key=250)
    L = _layout(H, W)
    D = _delta(k, L, x, eps, xt, None, None, 1)
    out = _step(k, x, eps, xt, z, D, g, 1)
    ew, ec = torch.full((H, W), 1.0 - g, device=DEV), (g * L).contiguous()
    ref, plain = torch.empty_like(x), torch.empty_like(x)
    st = _lib.stream_ptr(DEV)
    assert lib.sinddm_reverse_step_edit(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(ref), C.byref(k),
                                        _lib.ptr(ew), _lib.ptr(ec), B, 3, H * W, st) == 0
    assert lib.sinddm_reverse_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(plain), C.byref(k),
                                   x.numel(), st) == 0
    torch.cuda.synchronize()
    err, bound = max_abs(out.cpu(), ref.cpu()), _bound(ref)
    print(f"N=1 g={g} mode {k.mode}: layout step vs reverse_step_edit(1 - g, g L) max-abs {err:.3e} (bound {bound:.3e}); "
          f"to the unconditioned step {max_abs(out.cpu(), plain.cpu()):.3e}")
    assert err <= bound
    assert max_abs(out.cpu(), plain.cpu()) > 1e-2


# ---- 6: contraction on the device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,N", [(33, 50, 8), (48, 64, 4), (67, 90, 3), (25, 34, 16)])
def test_one_pull_contracts_the_low_band_on_the_device(diff20, H, W, N):
    k = diff20.step_coefs(0, 1, clip_denoised=False)
    assert k.mode == 2 and k.clip == 0 and k.sigma == 0.0
    x, eps, xt, z, _, _ = _inputs(2, H, W, key=350)
    L = _layout(H, W)
    D = _delta(k, L, x, eps, xt, None, None, N)
    out = _step(k, x, eps, xt, z, D, 1.0, N)                  # mode 2 without clamp: x_recon after the pull
    D2 = LU.block_mean(_np(L)[None] - _np(out), N)
    slack = _delta_bound(k, L, x, eps, xt, None, None, N)
    for b in range(2):
        n0, n1 = np.linalg.norm(_np(D)[b]), np.linalg.norm(D2[b])
        print(f"{H}x{W} N={N} sample {b}: ||M r'|| / ||M r|| = {n1 / n0:.3f} (bound 0.75)")
        assert n1 <= 0.75 * n0 + slack * np.sqrt(D2[b].size)


# ---- 7: fused equals stepwise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_fused_layout_equals_stepwise_layout(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    d, seed = c.d, 717171 + s
    L = _layout(c.H, c.W)
    assert ts[1] > ts[2] == 0
    d.layout_maps, d.layout_down, d.layout_strength, d.layout_t_min = {s: L}, {s: N_CHAIN}, 1.0, ts[1]      # g = (1, 1, 0)
    for with_keep in (False, True):
        for with_edit in (False, True):
            edit = (c.ew, c.ec) if with_edit else None
            keep = (c.m, c.k0) if with_keep else None
            d.roi_guided_sampling = with_edit
            d.keep_maps = {s: keep} if with_keep else None
            x = c.x0.clone()
            for i, t in enumerate(ts):
                z = c.centre(_draw(c, c.x0, seed, i))
                d.noise_fn = lambda kind, shape, ss, tt, dev, z=z: z
                x = d._p_sample_host_t(x, t, s)
            d.noise_fn = None
            y = _chain_lay(c, c.x0, ts, seed, aux=aux, edit=edit, keep=keep, lay=L)
            assert torch.isfinite(y).all()
            err, bound = max_abs(c.centre(y).cpu(), x.cpu()), _bound(x)
            print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B} keep={with_keep} edit={with_edit}: fused layout vs "
                  f"stepwise layout max-abs {err:.3e} (bound {bound:.3e})")
            assert err <= bound
            # the pull is not a no-op: the call without the option lands elsewhere
            y_plain = _chain_lay(c, c.x0, ts, seed, aux=aux, edit=edit, keep=keep, lo="null")
            assert max_abs(y_plain.cpu(), y.cpu()) > 1e-2
            if aux:
                assert torch.equal(y, _chain_lay(c, c.x0, ts, seed, aux=False, edit=edit, keep=keep, lay=L))
            if not with_keep and not with_edit:
                # the public route is exactly this call with the seed it drew
                torch.manual_seed(11)
                seed_api = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
                torch.manual_seed(11)
                d.two_streams = aux
                y_api = d._run_steps(c.x0.clone(), s, ts)
                assert torch.equal(y_api, c.centre(_chain_lay(c, c.x0, ts, seed_api, aux=aux, lay=L)))


# ---- 8: bit-level identities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_option_off_is_the_resample_entry(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    seed, L, keep = 434343 + s, _layout(c.H, c.W), (c.m, c.k0)
    y0 = _chain_lay(c, c.x0, ts, seed, aux=aux, keep=keep, entry="resample")
    assert torch.equal(y0, _chain_lay(c, c.x0, ts, seed, aux=aux, keep=keep, lo="null"))
    assert torch.equal(y0, _chain_lay(c, c.x0, ts, seed, aux=aux, keep=keep, lo="no_layout"))
    assert torch.equal(y0, _chain_lay(c, c.x0, ts, seed, aux=aux, keep=keep, lay=L, g=(0.0, 0.0, 0.0)))
    assert float(c.last_delta.min()) == 7.5 == float(c.last_delta.max())          # (the scratch was not written)


@pytest.mark.parametrize("B", [16, 18], ids=["B16", "B18_half_starts_inside_a_quad"])
def test_streams_rerun_and_noise_buffers(B):
    """67x90 (padded rows, two streams): one stream == two streams == re-run; the Philox run equals the run on buffers of
    sinddm_normal_fill[_samples] at the documented stream ids, unseeded and seeded.  At B = 18 the second half-batch starts at
    element 9 * 3 * 67 * 90 = 162810 = 2 mod 4 of the whole batch: inside a quad of the stream."""
    cfg, dim, s, _, aux, ts, hx = CASES[1]
    assert aux and hx == 0 and ((B + 1) // 2 * 3 * 67 * 90) % 4 == (0 if B == 16 else 2)
    c = _ctx(cfg, dim, s, B, 0)
    assert (c.H, c.W) == (67, 90)
    seed, sid0, L, keep = 868 + B, (s << 32) | 2, _layout(c.H, c.W), (c.m, c.k0)
    y2 = _chain_lay(c, c.x0, ts, seed, sid0=sid0, aux=True, keep=keep, lay=L)
    assert torch.equal(y2, _chain_lay(c, c.x0, ts, seed, sid0=sid0, aux=False, keep=keep, lay=L))
    assert torch.equal(y2, _chain_lay(c, c.x0, ts, seed, sid0=sid0, aux=True, keep=keep, lay=L))
    nz = torch.stack([_draw(c, c.x0, seed, sid0 + i) for i in range(len(ts))]).contiguous()
    assert torch.equal(y2, _chain_lay(c, c.x0, ts, 0, aux=True, keep=keep, lay=L, noise=nz))
    assert max_abs(y2.cpu(), _chain_lay(c, c.x0, ts, seed, sid0=sid0, aux=True, keep=keep, lo="null").cpu()) > 1e-2
    seeds = _seed_list(B)
    ys = _chain_lay(c, c.x0, ts, sid0=sid0, aux=True, keep=keep, lay=L, seeds=seeds)
    assert torch.equal(ys, _chain_lay(c, c.x0, ts, sid0=sid0, aux=False, keep=keep, lay=L, seeds=seeds))
    nzs = _sample_draws(c, c.x0, seeds, len(ts), sid0)
    assert torch.equal(ys, _chain_lay(c, c.x0, ts, aux=True, keep=keep, lay=L, noise=nzs))
    assert not torch.equal(ys, y2)


# ---- 9: batch position -------------------------------------------------------------------------------------------------------
def test_seeded_sample_at_any_position():
    cfg, dim, s, B, aux, ts, hx = CASES[1]                                      # pitch 67x90, two streams at batch 16
    big = _ctx(cfg, dim, s, 16, 0)
    sigma, pos16 = 0x1234567890ABCDEF & ((1 << 63) - 1), 12                     # position 12: the second half-batch
    sid0, L = (s << 32) | 2, _layout(big.H, big.W)
    x_one, xt_one = big.x0[pos16:pos16 + 1].clone(), big.xt[pos16:pos16 + 1].clone()
    k = big.d._coef_table(s)[ts[0]]
    eps_one = (hash_randn((1, 3, big.H, big.W), 444)).to(DEV)

    def run(B_, pos, aux_):
        c = _ctx(cfg, dim, s, B_, 0)
        c.x0, c.xt = big.x0[:B_].clone(), big.xt[:B_].clone()
        c.x0[pos], c.xt[pos] = x_one[0], xt_one[0]
        seeds = [1000 + 17 * b for b in range(B_)]
        seeds[pos] = sigma
        y = _chain_lay(c, c.x0, ts, sid0=sid0, aux=aux_, lay=L, seeds=seeds)
        nzs = _sample_draws(c, c.x0, seeds, len(ts), sid0)
        assert torch.equal(y, _chain_lay(c, c.x0, ts, aux=aux_, lay=L, noise=nzs))
        # D of the sample from the same state, whatever surrounds it
        eps = (hash_randn((B_, 3, c.H, c.W), 445) * 1.0).to(DEV)
        eps[pos] = eps_one[0]
        D = _delta(k, L, c.x0, eps, c.xt, None, None, N_CHAIN)
        return y[pos], nzs[:, pos], D[pos]

    y1, nz1, D1 = run(1, 0, False)
    for B_, pos, aux_ in ((3, 2, False), (16, pos16, True)):
        y, nz, D = run(B_, pos, aux_)
        assert torch.equal(nz, nz1)                                             # the noise: bit-equal
        assert torch.equal(D, D1)                                               # the block delta: bit-equal
        # the images: another batch size may take other convolution kernels, so the bound is the one test_gpu_seeds applies
        # across batch sizes, not the same-kernel bound
        err = rel_l2(y.cpu(), y1.cpu())
        print(f"seeded sample at position {pos} of {B_} (two streams={aux_}) vs batch of one: rel-L2 {err:.3e} (budget "
              f"{BUDGET:.0e}) max-abs {max_abs(y.cpu(), y1.cpu()):.3e} bit-equal {torch.equal(y, y1)}")
        assert err <= BUDGET


# ---- 10: error codes ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_device_work():
    from sinddm_amd import _lib
    from sinddm_amd.models import _workspace
    lib = _lib.load()
    c = _Ctx("C2", 20, 0, 2, 0)
    B, H, W, ts = 2, c.H, c.W, [700, 2]
    xa = c.x0.clone()
    xb, eps = torch.full_like(xa, 3.25), torch.full_like(xa, 4.5)
    L = _layout(H, W)
    delta = torch.full((B, 3, H, W), 7.5, device=DEV)          # (room for every block size down to 1)
    pad = torch.zeros(3 * H * W + 4, device=DEV)
    tab = c.d._coef_table(0)
    coefs = (_lib.StepCoefs * 2)(tab[700], tab[2])
    tl = (C.c_int * 2)(*ts)
    ws = _workspace(DEV, lib.sinddm_workspace_bytes(20, B, H, W))
    flag = C.c_int(7)

    def call(down=8, g=(1.0, 0.0), g_null=False, delta_ptr=_lib.ptr(delta), layout_ptr=_lib.ptr(L), jump_on=None):
        opts, lopts, rs = _lib.ChainOpts(), _lib.LayoutOpts(), _lib.ResampleOpts()
        garr = (C.c_float * 2)(*g)
        lopts.layout, lopts.down, lopts.delta = layout_ptr, down, delta_ptr
        lopts.g = None if g_null else C.cast(garr, C.POINTER(C.c_float))
        J = _lib.JumpCoefs
        jumps = (J * 2)(*[J(1, 0.8, 0.6, 0.0) if jump_on == i else J(0, 0.0, 0.0, 0.0) for i in range(2)])
        rs.jumps = C.cast(jumps, C.POINTER(J))
        return lib.sinddm_sample_chain_layout(
            _lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), None, coefs,
            tl, 2, 0.0, 1, 0, 20, B, H, W, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV), None, C.byref(flag), C.byref(opts),
            0, 0, None, None, C.byref(rs) if jump_on is not None else None, C.byref(lopts))

    bad = [dict(down=0), dict(down=65), dict(down=-3), dict(g=(1.0001, 0.0)), dict(g=(0.5, -0.1)), dict(g=(float("nan"), 0.0)),
           dict(g_null=True), dict(delta_ptr=None), dict(layout_ptr=pad.data_ptr() + 4), dict(jump_on=0)]
    for kw in bad:
        assert call(**kw) == -1, kw                                             # SINDDM_E_BADARG
    torch.cuda.synchronize()
    # none of these touched the device or the result flag
    assert flag.value == 7
    assert torch.equal(xa, c.x0) and float(xb.min()) == 3.25 == float(xb.max()) and float(eps.min()) == 4.5 == float(eps.max())
    assert float(delta.min()) == 7.5 == float(delta.max())
    # a jump on a step that is not conditioned is fine, and so are the ends of the ranges
    # a run without a positive strength reads nothing else of the block: it is the plain run
    assert call(down=0, g=(0.0, 0.0), delta_ptr=None, layout_ptr=pad.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    assert float(delta.min()) == 7.5 == float(delta.max())
    assert call(jump_on=1) == 0 and call(down=1, g=(1.0, 1.0)) == 0 and call(down=64) == 0
    torch.cuda.synchronize()
    assert float(delta.max()) != 7.5


# ---- 11: end to end on the C1 pyramid --------------------------------------------------------------------------------------------
def test_paint2image_on_c1(golden, tmp_path):
    from sinddm_amd.functions import _layout_pyramid
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    sizes = [tuple(s) for s in meta["image_sizes_hw"]]
    H, W = sizes[-1]
    lay = (hash_randn((3, H, W), 909) * 0.8).clamp(-1, 1)
    tl, seeds = em.num_timesteps_ideal[1:], [5, 6]
    # strength 0 is sample_scales
    a = tr.paint2image(lay, batch_size=2, strength=0.0, seeds=seeds, custom_t_list=tl, save_images=False)
    b = tr.sample_scales(batch_size=2, seeds=seeds, custom_t_list=tl, save_images=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert em.layout_maps is None and em.layout_down == {}
    # block size 1 at full strength on every step: every scale ends on its clamped layout, whatever the network says
    em.draw_log = []
    outs = tr.paint2image(lay, batch_size=2, down=1, strength=1.0, t_min=0, seeds=seeds, custom_t_list=tl, save_images=False)
    log, em.draw_log = em.draw_log, None
    assert [e[0] for e in log if e[0].startswith("chain")] == ["chain_seeds"] * len(sizes)      # one chain call per scale
    pyr = _layout_pyramid(lay, sizes)
    for s_, (o, p) in enumerate(zip(outs, pyr)):
        ref = p.clamp(-1, 1).to(DEV)[None].expand_as(o)
        err = max_abs(o.cpu(), ref.cpu())
        print(f"paint2image down=1 strength=1 scale {s_} {tuple(o.shape)}: max-abs to the clamped layout {err:.3e} "
              f"(bound {_bound(ref):.3e})")
        assert err <= _bound(ref)
    assert max_abs(outs[-1].cpu(), b[-1].cpu()) > 1e-2
    # a loose pull follows the layout's low band and differs between samples
    outs = tr.paint2image(lay, batch_size=2, down=8, strength=1.0, t_min=2, scales=(1, len(sizes) - 1), custom_t_list=tl,
                          save_images=False)
    assert all(torch.isfinite(o).all() for o in outs) and max_abs(outs[-1][0].cpu(), outs[-1][1].cpu()) > 1e-2
    # tiled
    em.tile = (False, True)
    outs = tr.paint2image(lay, batch_size=2, down=8, custom_t_list=tl, save_images=False)
    em.tile = (False, False)
    assert [tuple(o.shape) for o in outs] == [(2, 3) + hw for hw in sizes] and all(torch.isfinite(o).all() for o in outs)
    # with resampling jumps it is refused, and the attributes are put back
    em.resample = (2, 1)
    with pytest.raises(NotImplementedError):
        tr.paint2image(lay, batch_size=2, custom_t_list=tl, save_images=False)
    em.resample = None
    assert em.layout_maps is None and em.layout_down == {} and em.layout_strength == 1.0 and em.layout_t_min == 0
