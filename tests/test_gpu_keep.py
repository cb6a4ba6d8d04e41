"""Known-region conditioning inside the fused sampler chain (sinddm_sample_chain_keep / sinddm_reverse_step_keep): after every
reverse step the pixels a mask marks as known are overwritten with the forward-diffused known image of that noise level
(RePaint-style replacement; inpainting and outpainting), in the four step-tail kernels.

The reference has no counterpart, so the yardsticks are exactness properties and the project's own step-by-step route:
  1. the fused chain equals the step-by-step route (sinddm_net_forward + sinddm_reverse_step_keep) on every tail kernel, with
     and without ROI edit maps; one and two streams are bit-equal; `_run_steps` is the direct call;
  2. exact ends: m == 0 is the call without keep, m == 1 ending at t = 0 returns the known image, both bit for bit;
  3. known pixels do not depend on the network: after each step they are keep_a * target + keep_b * z of the same z, and
     unknown pixels are the plain call's, bit for bit;
  4. a noise buffer holding the Philox stream's numbers reproduces the Philox run bit for bit, keep on;
  5. sinddm_reverse_step_keep against the blend assembled in torch, modes 0, 1, 2;
  6. `inpaint` / `outpaint` on the C1 pyramid: one chain per scale, kept pixels exact, the hole differs between samples.
Shapes: the four of test_gpu_chain_guided.SHAPES (each reaches one tail kernel; three steps incl. t = 0) and one tiled case.
"""
import ctypes as C

import pytest
import torch

from conftest import max_abs
from sinddm_amd.synth import hash_randn
from test_gpu_chain_guided import IDS, SHAPES, _fill, _setup, _trainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (cfg, dim, s, B, two streams, steps, halo_x): the tiled case runs 48x64 extended to 48x96 (plain fused tail)
CASES = [sh + (0,) for sh in SHAPES] + [("C2", 160, 0, 16, False, [700, 2, 0], 16)]
CASE_IDS = IDS + ["tiled_48x64_halo_x16"]


def _mask(H, W):
    """Edges off the quad grid, a soft region written second (it overrides the overlap), contact with two borders."""
    m = torch.zeros(H, W)
    m[5:25, 8:32] = 1
    m[14:31, 13:43] = 0.25
    m[H - 11:, W - 9:] = 1
    return m.to(DEV)


def _known(H, W, key=70):
    return (hash_randn((3, H, W), key) * 0.6).clamp(-1, 1).to(DEV)


class _Ctx:
    """One shape: diffusion, centre-size inputs / maps and their extended (wrapped) versions for the library call."""

    def __init__(self, cfg, dim, s, B, hx):
        self.net, self.d, self.H, self.W, self.x0, self.xt, self.ew, self.ec = _setup(cfg, dim, s, B)
        self.s, self.dim, self.hx = s, dim, hx
        if s == 0:
            self.xt = None                                   # (mode 0 everywhere: no x-tilde)
        self.m, self.k0 = _mask(self.H, self.W), _known(self.H, self.W)
        self.d.tile = (False, bool(hx))

    def ext(self, t):
        return None if t is None else (self.d._wrap_pad(t, 0, self.hx) if self.hx else t.contiguous())

    def centre(self, t):
        return t[..., self.hx:self.hx + self.W].contiguous() if self.hx else t


def _chain(c, x0, ts, seed, sid0=0, aux=False, edit=None, noise=None, keep=None, entry="keep"):
    """sinddm_sample_chain_keep (or _tile) on centre-size arguments, extended here; returns (rc, extended result)."""
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
    held = []                                               # (extended maps: alive until the synchronise below)
    if edit is not None:
        held += [c.ext(edit[0]), c.ext(edit[1])]
        opts.edit_w, opts.edit_c = _lib.ptr(held[0]), _lib.ptr(held[1])
    opts.noise = _lib.ptr(noise)
    args = [_lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
            coefs, tl, n, float(c.s), seed, sid0, c.dim, B, H, We - 2 * c.hx, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
            _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, c.hx]
    if entry == "keep":
        kopts = None
        if keep is not None:
            held += [c.ext(keep[0]), c.ext(keep[1])]
            ab_tab = c.d._keep_ab_table()
            ab = (C.c_float * (2 * n))(*[float(v) for t in ts for v in ab_tab[t]])
            kopts = _lib.KeepOpts()
            kopts.mask, kopts.x0, kopts.ab = _lib.ptr(held[-2]), _lib.ptr(held[-1]), C.cast(ab, C.POINTER(C.c_float))
        rc = lib.sinddm_sample_chain_keep(*args, C.byref(kopts) if kopts is not None else None)
    else:
        assert keep is None
        rc = lib.sinddm_sample_chain_tile(*args)
    torch.cuda.synchronize()
    assert rc == 0 and flag.value in (0, 1)
    return xb if flag.value == 1 else xa


def _draw(c, x0, seed, i):
    """Draw i of a run as the chain's kernels see it: over the EXTENDED tensor."""
    shape = tuple(x0.shape[:3]) + (x0.shape[3] + 2 * c.hx,)
    n = 1
    for v in shape:
        n *= v
    return _fill(n, seed, i).view(shape)


def _bound(ref):
    return 4e-6 * max(1.0, float(ref.abs().max()))          # the bound of test_fused_edit_equals_stepwise_edit


# ---- 1: fused equals stepwise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_edit", [False, True], ids=["keep", "keep_edit"])
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_fused_keep_equals_stepwise_keep(cfg, dim, s, B, aux, ts, hx, with_edit):
    c = _Ctx(cfg, dim, s, B, hx)
    d, seed = c.d, 616161 + s
    edit = (c.ew, c.ec) if with_edit else None
    d.roi_guided_sampling = with_edit
    d.keep_maps = {s: (c.m, c.k0)}
    x = c.x0.clone()
    for i, t in enumerate(ts):
        z = c.centre(_draw(c, c.x0, seed, i))
        d.noise_fn = lambda kind, shape, ss, tt, dev, z=z: z
        x = d._p_sample_host_t(x, t, s)
    d.noise_fn = None
    y = _chain(c, c.x0, ts, seed, aux=aux, edit=edit, keep=(c.m, c.k0))
    assert torch.isfinite(y).all()
    err, bound = max_abs(c.centre(y).cpu(), x.cpu()), _bound(x)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B} edit={with_edit}: fused keep vs stepwise keep max-abs "
          f"{err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # the keep is not a no-op: the call without it lands elsewhere
    y_plain = _chain(c, c.x0, ts, seed, aux=aux, edit=edit)
    assert max_abs(y_plain.cpu(), y.cpu()) > 1e-2
    if aux:
        assert torch.equal(y, _chain(c, c.x0, ts, seed, aux=False, edit=edit, keep=(c.m, c.k0)))
    # ... and the public route is exactly this call with the seed it drew
    torch.manual_seed(11)
    seed_api = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
    torch.manual_seed(11)
    d.two_streams = aux
    d.draw_log = []
    y_api = d._run_steps(c.x0.clone(), s, ts)
    log, d.draw_log = d.draw_log, None
    assert len(log) == 1 and log[0][0] == ("chain_tile" if hx else "chain") and log[0][2] == seed_api       # entries unchanged
    assert torch.equal(y_api, c.centre(_chain(c, c.x0, ts, seed_api, aux=aux, edit=edit, keep=(c.m, c.k0))))


# ---- 2: exact ends -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_keep_exact_ends(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    seed = 424242 + s
    y_tile = _chain(c, c.x0, ts, seed, aux=aux, entry="tile")
    assert torch.equal(_chain(c, c.x0, ts, seed, aux=aux), y_tile)                  # keep = NULL is the tile entry itself
    y0 = _chain(c, c.x0, ts, seed, aux=aux, keep=(torch.zeros_like(c.m), c.k0))
    assert torch.equal(y0, y_tile)                                                  # m == 0: the plain step, bit for bit
    assert ts[-1] == 0
    y1 = _chain(c, c.x0, ts, seed, aux=aux, keep=(torch.ones_like(c.m), c.k0))
    assert torch.equal(c.centre(y1), c.k0[None].expand(B, -1, -1, -1))              # m == 1 down to t = 0: the known image


# ---- 3: known pixels do not depend on the network ----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_known_pixels_do_not_depend_on_the_network(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    seed = 909090 + s
    tab, ab = c.d._coef_table(s), c.d._keep_ab_table()
    known, unknown = (c.m == 1).expand(B, 3, -1, -1), (c.m == 0).expand(B, 3, -1, -1)
    assert bool(known.any()) and bool(unknown.any()) and bool(((c.m > 0) & (c.m < 1)).any())
    x = c.x0
    for i, t in enumerate(ts):
        y = c.centre(_chain(c, x, [t], seed, sid0=i, aux=aux, keep=(c.m, c.k0)))
        plain = c.centre(_chain(c, x, [t], seed, sid0=i, aux=aux, entry="tile"))
        z = c.centre(_draw(c, x, seed, i)).double()
        k = tab[t]
        target = c.k0.double()[None]
        if k.mode == 1:
            target = float(k.gamma_tm1) * c.xt.double() + (1.0 - float(k.gamma_tm1)) * target
        kept = float(ab[t][0]) * target + float(ab[t][1]) * z
        err, bound = float((y.double() - kept)[known].abs().max()), _bound(kept)
        print(f"{cfg} dim {dim} s={s} halo_x={hx} t={t} mode {k.mode}: known pixels vs keep_a*target + keep_b*z max-abs "
              f"{err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert torch.equal(y[unknown], plain[unknown])
        assert max_abs(y[known].cpu(), plain[known].cpu()) > 1e-2               # (the known pixels did move)
        x = y


# ---- 4: noise handling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_keep_noise_buffer_equals_philox(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    seed, sid0 = 787 + s, 5
    assert c.d._coef_table(s)[ts[-1]].sigma == 0.0                              # the run includes a step without noise
    y0 = _chain(c, c.x0, ts, seed, sid0=sid0, aux=aux, keep=(c.m, c.k0))
    draws = lambda sd: torch.stack([_draw(c, c.x0, sd, sid0 + i) for i in range(len(ts))]).contiguous()
    y1 = _chain(c, c.x0, ts, 0, aux=aux, keep=(c.m, c.k0), noise=draws(seed))
    assert torch.equal(y0, y1)
    y2 = _chain(c, c.x0, ts, 0, aux=aux, keep=(c.m, c.k0), noise=draws(seed + 1))
    assert not torch.equal(y0, y2)                                              # the buffer is what is read


# ---- 5: the stepwise kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,t", [(0, 700), (1, 400), (1, 0)], ids=["mode0", "mode1", "mode2"])
def test_reverse_step_keep_against_torch(s, t):
    from sinddm_amd import _lib
    from sinddm_amd.configs import build_diffusion
    lib = _lib.load()
    net, d = build_diffusion("C2", dim=20, device=DEV)
    B, H, W = 3, 37, 45                                                         # odd sizes, several blocks
    x, eps, xt, z = ((hash_randn((B, 3, H, W), 50 + i) * a).to(DEV) for i, a in enumerate((0.8, 1.0, 0.5, 1.0)))
    m, k0 = _mask(H, W), _known(H, W, 71)
    ew = (0.2 + 0.8 * hash_randn((H, W), 60).abs().clamp(0, 1)).to(DEV)
    ec = (hash_randn((3, H, W), 61) * 0.3).to(DEV)
    k = d.step_coefs(t, s)
    assert k.mode == {(0, 700): 0, (1, 400): 1, (1, 0): 2}[(s, t)]
    st = _lib.stream_ptr(DEV)
    for edit in (False, True):
        plain = torch.empty_like(x)
        if edit:
            rc = lib.sinddm_reverse_step_edit(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(plain), C.byref(k),
                                              _lib.ptr(ew), _lib.ptr(ec), B, 3, H * W, st)
        else:
            rc = lib.sinddm_reverse_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(plain), C.byref(k),
                                         x.numel(), st)
        assert rc == 0
        # the schedule's own scalars, and a pair with keep_b != 0 at every mode (t = 0 has keep_b = 0)
        for ka, kb in (tuple(float(v) for v in d._keep_ab_table()[t]), (0.8, 0.6)):
            out = torch.empty_like(x)
            rc = lib.sinddm_reverse_step_keep(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(out), C.byref(k),
                                              _lib.ptr(ew) if edit else None, _lib.ptr(ec) if edit else None, _lib.ptr(m),
                                              _lib.ptr(k0), ka, kb, B, 3, H * W, st)
            torch.cuda.synchronize()
            assert rc == 0
            target = k0[None].expand_as(x)
            if k.mode == 1:
                target = k.gamma_tm1 * xt + (1.0 - k.gamma_tm1) * target
            ref = m * (ka * target + kb * z) + (1 - m) * plain
            err, bound = max_abs(out.cpu(), ref.cpu()), _bound(ref)
            print(f"s={s} t={t} mode {k.mode} edit={edit} (keep_a, keep_b)=({ka:.4f}, {kb:.4f}): reverse_step_keep vs torch "
                  f"max-abs {err:.3e} (bound {bound:.3e})")
            assert err <= bound
            sel = (m == 0).expand_as(x)
            assert torch.equal(out[sel], plain[sel])                            # exact at m == 0


# ---- 6: end to end on the C1 pyramid ---------------------------------------------------------------------------------------------
def test_inpaint_and_outpaint_on_c1(golden, tmp_path):
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    sizes = [tuple(s) for s in meta["image_sizes_hw"]]
    H, W = sizes[-1]
    img = tr.data_list[-1][0][0]
    mask = torch.ones(H, W)
    mask[31:61, 43:83] = 0                                                      # a 30x40 hole
    em.draw_log = []
    torch.manual_seed(2468)
    outs = tr.inpaint(mask, batch_size=2, custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    log, em.draw_log = em.draw_log, None
    assert em.keep_maps is None
    assert [e[0] for e in log] == ["init", "chain", "renoise", "chain", "renoise", "chain"]      # one chain per scale
    assert [tuple(o.shape) for o in outs] == [(2, 3) + hw for hw in sizes]
    assert all(torch.isfinite(o).all() for o in outs)
    kept = mask.bool().to(DEV)
    assert torch.equal(outs[-1][:, :, kept], img[None].expand(2, -1, -1, -1)[:, :, kept])       # the kept pixels, exactly
    diff = max_abs(outs[-1][0][:, ~kept].cpu(), outs[-1][1][:, ~kept].cpu())
    print(f"inpaint C1 dim 32 T=20 B=2: the two samples differ inside the hole by max-abs {diff:.3e}")
    assert diff > 1e-2
    # soft masks and a raised error both put keep_maps back
    tr.inpaint(mask, batch_size=2, hard=False, custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    with pytest.raises(ValueError):
        tr.inpaint(mask[:-1], batch_size=2, save_images=False)
    assert em.keep_maps is None
    # outpaint: the canvas grows to 1.5 x the width, the training image sits centred and unresampled
    outs = tr.outpaint((1, 1.5), batch_size=2, custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    assert em.keep_maps is None
    assert [tuple(o.shape) for o in outs] == [(2, 3, h, int(w * 1.5)) for h, w in sizes]
    x0 = int(0.5 * (int(W * 1.5) - W))
    assert torch.equal(outs[-1][:, :, :, x0:x0 + W], img[None].expand(2, -1, -1, -1))
    side = max_abs(outs[-1][0][:, :, :x0].cpu(), outs[-1][1][:, :, :x0].cpu())
    assert torch.isfinite(outs[-1]).all() and side > 1e-2                       # the new canvas is generated, per sample
    with pytest.raises(ValueError):
        tr.outpaint((1, 0.9), batch_size=2, save_images=False)
