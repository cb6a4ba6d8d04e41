"""RePaint's resampling jumps inside the fused sampler chain (sinddm_sample_chain_resample / sinddm_reverse_step_jump): a step
that is followed by a jump runs unfused (the network writes eps) and ends in ONE elementwise kernel that does the reverse
step and the upward move of SinDDM's blurred forward process, with a second N(0,1) draw from the stream
`step + SINDDM_JUMP_STREAM`.

The reference has no counterpart, so the yardsticks are a float64 restatement of the formulas (tests/resample_util.py), the
project's own step-by-step route, bit-level identities and the marginal the jump must land on:
  4. sinddm_reverse_step_jump against the float64 restatement (modes 0 / 1, keep and edit off / on, two odd sizes);
  5. the fused chain with caller noise equals the same schedule driven step by step, keep on, with and without edit;
  6. identities, bit for bit: no jumps = sinddm_sample_chain_seeds; one stream = two streams; a run repeats; noise buffers
     holding the documented Philox streams reproduce the in-kernel run, unseeded and seeded;
  7. the seeds contract through a resampled chain: batch of one, position 2 of 3, second half of a two-stream run (noise
     bit-equal, images within the budget test_gpu_seeds applies across batch sizes);
  8. the marginal after step + jump under a full mask (catches a reused draw);
  9. `MultiscaleTrainer.inpaint(resample=2, jump_length=2)` on the C1 pyramid.
Shapes: the four of test_gpu_chain_guided.SHAPES (one per tail kernel / row layout, two streams on one) and the tiled
48x64 case of test_gpu_keep.CASES; five evaluations each: [t, t-1] ^t [t, t-1] [0] -- a jump of two levels between two
arithmetic runs of t, and a last run that ends at t = 0.
"""
import ctypes as C

import pytest
import torch

from conftest import max_abs, rel_l2
from resample_util import closed_form_count, moment_limits, step_jump_ref, whitened
from sinddm_amd.synth import hash_randn
from test_gpu_chain_guided import _trainer
from test_gpu_keep import CASE_IDS, CASES, _bound, _draw
from test_gpu_seeds import BUDGET, _chain_seeds, _ctx, _dev_seeds, _seed_list

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
JS = 1 << 31                                                    # SINDDM_JUMP_STREAM


# the first step of a scale's walk: below the level at which the scale's sampling gamma saturates at 0.55 (C2: about 340 at
# scale 1, 185 at scale 3), so that gamma differs between the two ends of the jump and its d term is at work
T_OF = {0: 700, 1: 200, 3: 100}


def _walk(s):
    """The five-evaluation walk of a shape: (t list, jump target per step)."""
    t = T_OF[s]
    return [t, t - 1, t, t - 1, 0], [None, t, None, None, None]


RS_CASES = [(cfg, dim, s, B, aux) + _walk(s) + (hx,) for cfg, dim, s, B, aux, ts, hx in CASES]
# a two-stream run whose second half starts INSIDE a quad of the whole batch's stream: 9 * 3 * 67 * 90 % 4 == 2
UNALIGNED = ("C2", 160, 1, 18, True) + _walk(1) + (0,)


def _jump_array(c, ts, jump_to):
    from sinddm_amd import _lib
    jt = c.d._jump_table(c.s)
    return (_lib.JumpCoefs * len(ts))(*[_lib.JumpCoefs(0, 0.0, 0.0, 0.0) if l2 is None else _lib.JumpCoefs(1, *jt(t - 1, l2))
                                        for t, l2 in zip(ts, jump_to)])


def _chain_rs(c, x0, ts, jump_to, seed=0, sid0=0, aux=False, edit=None, keep=None, noise=None, jnoise=None, seeds=None,
              rs="jumps", expect_rc=0):
    """sinddm_sample_chain_resample on centre-size arguments of a test_gpu_keep._Ctx, extended here; the extended result.
    rs: "jumps" (the walk's jumps), "off" (an array with no entry on) or "null" (rs = NULL)."""
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
    ropts = None
    if rs != "null":
        jumps = _jump_array(c, ts, jump_to if rs == "jumps" else [None] * n)
        ropts = _lib.ResampleOpts()
        ropts.jumps, ropts.noise = C.cast(jumps, C.POINTER(_lib.JumpCoefs)), _lib.ptr(jnoise)
    rc = lib.sinddm_sample_chain_resample(
        _lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
        coefs, tl, n, float(c.s), seed, sid0, c.dim, B, H, We - 2 * c.hx, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
        _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, c.hx,
        C.byref(kopts) if kopts is not None else None, _lib.ptr(sd), C.byref(ropts) if ropts is not None else None)
    torch.cuda.synchronize()
    assert rc == expect_rc
    if rc != 0:
        return None
    assert flag.value in (0, 1)
    return xb if flag.value == 1 else xa


def _buffers(c, x0, ts, jump_to, seed, sid0):
    """(opts->noise, rs->noise) holding what the in-kernel streams give an UNSEEDED run: step i reads
    sinddm_normal_fill(n_total, seed, sid0 + i), the jump after it sinddm_normal_fill(n_total, seed, sid0 + i + 2^31); over
    the extended tensor."""
    nz = torch.stack([_draw(c, x0, seed, sid0 + i) for i in range(len(ts))]).contiguous()
    jn = torch.stack([_draw(c, x0, seed, sid0 + i + JS) for i, l2 in enumerate(jump_to) if l2 is not None]).contiguous()
    return nz, jn


def _sample_buffers(c, x0, ts, jump_to, seeds, sid0):
    """The same for a SEEDED run: sample b of step i is sinddm_normal_fill(3 H W, seeds[b], sid0 + i [+ 2^31]) over the
    extended sample (sinddm_normal_fill_samples)."""
    from sinddm_amd import _lib
    lib = _lib.load()
    B, Cc, H, W = x0.shape
    shape = (B, Cc, H, W + 2 * c.hx)
    sd = _dev_seeds(seeds)

    def fill(sid):
        out = torch.empty(shape, device=DEV)
        _lib.check(lib.sinddm_normal_fill_samples(_lib.ptr(out), B, out.numel() // B, _lib.ptr(sd), sid, _lib.stream_ptr(DEV)),
                   "sinddm_normal_fill_samples")
        return out

    nz = torch.stack([fill(sid0 + i) for i in range(len(ts))]).contiguous()
    jn = torch.stack([fill(sid0 + i + JS) for i, l2 in enumerate(jump_to) if l2 is not None]).contiguous()
    return nz, jn


# ---- 4: the stepwise kernel against the float64 restatement ------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (8, 12)], ids=["5x7", "8x12"])
@pytest.mark.parametrize("s,t,l2", [(0, 700, 709), (1, 200, 201), (1, 200, 209)], ids=["mode0", "mode1_J2", "mode1_J10"])
def test_reverse_step_jump_against_float64(s, t, l2, H, W):
    from sinddm_amd import _lib
    from sinddm_amd.configs import build_diffusion
    lib = _lib.load()
    net, d = build_diffusion("C2", dim=20, device=DEV)
    d.omega = 0.3                                                               # (a step sigma that shows: see test_gpu_seeds._ctx)
    B = 2
    assert (3 * H * W) % 4 == (1 if (H, W) == (5, 7) else 0)
    x, eps, xt, z, z2 = ((hash_randn((B, 3, H, W), 150 + i) * a).to(DEV) for i, a in enumerate((0.8, 1.0, 0.5, 1.0, 1.0)))
    m = torch.zeros(H, W)
    m[1:4, 2:6] = 1
    m[3:, 4:] = 0.25
    m, k0 = m.to(DEV), (hash_randn((3, H, W), 171) * 0.6).clamp(-1, 1).to(DEV)
    ew = (0.2 + 0.8 * hash_randn((H, W), 160).abs().clamp(0, 1)).to(DEV)
    ec = (hash_randn((3, H, W), 161) * 0.3).to(DEV)
    k = d.step_coefs(t, s)
    assert k.mode == (0 if s == 0 else 1)
    jc = _lib.JumpCoefs(1, *d._jump_table(s)(t - 1, l2))
    assert 0 < jc.r < 1 and jc.s > 0 and (jc.d != 0) == (s > 0)
    ka, kb = (float(v) for v in d._keep_ab_table()[t])
    st = _lib.stream_ptr(DEV)
    xt_arg = xt if s > 0 else None
    for keep in (False, True):
        for edit in (False, True):
            guard = 7.5
            buf = torch.full((x.numel() + 8,), guard, device=DEV)               # (the last quad must not write past the end)
            rc = lib.sinddm_reverse_step_jump(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt_arg), _lib.ptr(z), _lib.ptr(z2), _lib.ptr(buf),
                                              C.byref(k), C.byref(jc), _lib.ptr(ew) if edit else None,
                                              _lib.ptr(ec) if edit else None, _lib.ptr(m) if keep else None,
                                              _lib.ptr(k0) if keep else None, ka, kb, B, 3, H * W, st)
            torch.cuda.synchronize()
            assert rc == 0
            assert bool((buf[x.numel():] == guard).all())
            out = buf[:x.numel()].view_as(x)
            ref = step_jump_ref(d, s, t, l2, x, eps, xt_arg, z, z2, edit=(ew, ec) if edit else None,
                                keep=(m, k0) if keep else None)
            err, bound = float((out.cpu().double() - ref).abs().max()), 4e-6 * max(1.0, float(ref.abs().max()))
            print(f"s={s} t={t} -> level {l2} {H}x{W} keep={keep} edit={edit}: reverse_step_jump vs float64 max-abs {err:.3e} "
                  f"(bound {bound:.3e})")
            assert err <= bound
            # the jump is not a no-op: the step alone lands elsewhere
            alone = step_jump_ref(d, s, t, None, x, eps, xt_arg, z, z2, edit=(ew, ec) if edit else None,
                                  keep=(m, k0) if keep else None)
            assert float((alone - ref).abs().max()) > 1e-2
    # a jump after a mode-2 step does not exist
    k2 = d.step_coefs(0, 1)
    assert k2.mode == 2
    out = torch.empty_like(x)
    assert lib.sinddm_reverse_step_jump(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(z2), _lib.ptr(out),
                                        C.byref(k2), C.byref(jc), None, None, None, None, 1.0, 0.0, B, 3, H * W, st) == -1


# ---- 5: fused equals stepwise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_edit", [False, True], ids=["keep", "keep_edit"])
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,jump_to,hx", RS_CASES, ids=CASE_IDS)
def test_fused_resample_equals_stepwise(cfg, dim, s, B, aux, ts, jump_to, hx, with_edit):
    c = _ctx(cfg, dim, s, B, hx)
    d, seed = c.d, 717171 + s
    assert s == 0 or _jump_array(c, ts, jump_to)[1].d != 0.0                     # (the d term is at work)
    edit = (c.ew, c.ec) if with_edit else None
    d.roi_guided_sampling = with_edit
    d.keep_maps = {s: (c.m, c.k0)}
    nz, jn = _buffers(c, c.x0, ts, jump_to, seed, 0)
    x = c.x0.clone()
    nj = 0
    for i, (t, l2) in enumerate(zip(ts, jump_to)):
        draws = {"step": c.centre(nz[i])}
        if l2 is not None:
            draws["jump"] = c.centre(jn[nj])
            nj += 1
        d.noise_fn = lambda kind, shape, ss, tt, dev, draws=draws: draws[kind]
        x = d._p_sample_host_t(x, t, s, step_pos=i, jump_to=l2)
    d.noise_fn = None
    y = _chain_rs(c, c.x0, ts, jump_to, aux=aux, edit=edit, keep=(c.m, c.k0), noise=nz, jnoise=jn)
    assert torch.isfinite(y).all()
    err, bound = max_abs(c.centre(y).cpu(), x.cpu()), _bound(x)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B} edit={with_edit}: fused resample vs stepwise max-abs {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound
    # the jump is not a no-op: the same steps without it land elsewhere
    y_plain = _chain_rs(c, c.x0, ts, jump_to, aux=aux, edit=edit, keep=(c.m, c.k0), noise=nz, rs="off")
    assert max_abs(y_plain.cpu(), y.cpu()) > 1e-2
    # caller noise for the steps but none for the jumps is refused before anything runs
    _chain_rs(c, c.x0, ts, jump_to, aux=aux, keep=(c.m, c.k0), noise=nz, expect_rc=-1)
    # ... and `_run_steps` with chain_noise is this call, fed the same draws in the same order: the run [t, t-1, t-2] with
    # (R, J) = (2, 2) has one anchor (t - 2 or t - 3, the even one) and five or six evaluations
    from sinddm_amd.functions import resample_schedule
    run = [ts[0], ts[0] - 1, ts[0] - 2]
    walk, walk_to = resample_schedule(run, 2, 2)
    assert len(walk) in (5, 6) and sum(l2 is not None for l2 in walk_to) == 1
    nz2, jn2 = _buffers(c, c.x0, walk, walk_to, seed + 1, 0)
    fetched = []

    def fn(kind, shape, ss, tt, dev):
        fetched.append(kind)
        return c.centre(nz2[fetched.count("step") - 1]) if kind == "step" else c.centre(jn2[fetched.count("jump") - 1])

    d.noise_fn, d.chain_noise, d.two_streams, d.resample = fn, True, aux, (2, 2)
    y_api = d._run_steps(c.x0.clone(), s, run)
    d.noise_fn, d.chain_noise, d.resample = None, False, None
    assert fetched == [k for l2 in walk_to for k in (("step", "jump") if l2 is not None else ("step",))]
    ref_api = _chain_rs(c, c.x0, walk, walk_to, aux=aux, edit=edit, keep=(c.m, c.k0), noise=nz2, jnoise=jn2)
    assert torch.equal(y_api, c.centre(ref_api))


# ---- 6: identities, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,jump_to,hx", RS_CASES, ids=CASE_IDS)
def test_no_jumps_is_the_seeds_entry(cfg, dim, s, B, aux, ts, jump_to, hx):
    c = _ctx(cfg, dim, s, B, hx)
    keep, edit = (c.m, c.k0), (c.ew, c.ec)
    for seeds in (None, _seed_list(B)):
        ref = _chain_seeds(c, c.x0, ts, seeds, sid0=3, aux=aux, edit=edit, keep=keep, seed=55)
        for rs in ("null", "off"):
            y = _chain_rs(c, c.x0, ts, jump_to, seed=55, sid0=3, aux=aux, edit=edit, keep=keep, seeds=seeds, rs=rs)
            assert torch.equal(y, ref), (seeds is not None, rs)


@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,jump_to,hx", RS_CASES + [UNALIGNED], ids=CASE_IDS + ["pitch_67x90_B18_unaligned_half"])
def test_resample_noise_buffers_equal_philox(cfg, dim, s, B, aux, ts, jump_to, hx):
    """In-kernel Philox == buffers filled with the documented streams, unseeded (whole-batch index) and seeded (per-sample
    index); with a second stream == without; a run repeats; the jump's draw is its own."""
    c = _ctx(cfg, dim, s, B, hx)
    keep = (c.m, c.k0)
    seed, sid0 = 787 + s, (s << 32) | 2
    y0 = _chain_rs(c, c.x0, ts, jump_to, seed=seed, sid0=sid0, aux=aux, keep=keep)
    assert torch.isfinite(y0).all()
    assert torch.equal(y0, _chain_rs(c, c.x0, ts, jump_to, seed=seed, sid0=sid0, aux=aux, keep=keep))          # repeats
    if aux:
        assert torch.equal(y0, _chain_rs(c, c.x0, ts, jump_to, seed=seed, sid0=sid0, aux=False, keep=keep))    # one stream
    nz, jn = _buffers(c, c.x0, ts, jump_to, seed, sid0)
    y1 = _chain_rs(c, c.x0, ts, jump_to, aux=aux, keep=keep, noise=nz, jnoise=jn)
    same = torch.equal(y0, y1)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B}: Philox vs buffers max-abs {max_abs(y0.cpu(), y1.cpu()):.3e} "
          f"bit-equal {same}")
    assert same
    # the jump reads ITS buffer: with the step's own draw in its place the result moves
    y2 = _chain_rs(c, c.x0, ts, jump_to, aux=aux, keep=keep, noise=nz, jnoise=nz[1:2].contiguous())
    assert max_abs(y2.cpu(), y0.cpu()) > 1e-2
    # seeded
    seeds = _seed_list(B)
    ys = _chain_rs(c, c.x0, ts, jump_to, seed=999, sid0=sid0, aux=aux, keep=keep, seeds=seeds)      # (`seed` is ignored)
    if aux:
        assert torch.equal(ys, _chain_rs(c, c.x0, ts, jump_to, sid0=sid0, aux=False, keep=keep, seeds=seeds))
    nzs, jns = _sample_buffers(c, c.x0, ts, jump_to, seeds, sid0)
    ys1 = _chain_rs(c, c.x0, ts, jump_to, aux=aux, keep=keep, noise=nzs, jnoise=jns)
    print(f"    seeded: max-abs {max_abs(ys.cpu(), ys1.cpu()):.3e} bit-equal {torch.equal(ys, ys1)}")
    assert torch.equal(ys, ys1)
    assert max_abs(ys.cpu(), y0.cpu()) > 1e-2


# ---- 7: the seeds contract ---------------------------------------------------------------------------------------------------
def test_seeded_sample_through_a_resampled_chain_at_any_position():
    cfg, dim, s, B, aux, ts, jump_to, hx = RS_CASES[1]                          # pitch 67x90, two streams at batch 16
    assert aux and B == 16 and hx == 0
    big = _ctx(cfg, dim, s, B, 0)
    sigma, pos16 = 0x1234567890ABCDEF & ((1 << 63) - 1), 12                     # position 12: the second half-batch
    keep, sid0 = (big.m, big.k0), (s << 32) | 2
    x_one, xt_one = big.x0[pos16:pos16 + 1].clone(), big.xt[pos16:pos16 + 1].clone()

    def run(B_, pos, aux_):
        c = _ctx(cfg, dim, s, B_, 0)
        c.m, c.k0 = big.m, big.k0
        c.x0, c.xt = big.x0[:B_].clone(), big.xt[:B_].clone()
        c.x0[pos], c.xt[pos] = x_one[0], xt_one[0]
        seeds = [1000 + 17 * b for b in range(B_)]
        seeds[pos] = sigma
        y = _chain_rs(c, c.x0, ts, jump_to, sid0=sid0, aux=aux_, keep=keep, seeds=seeds)
        nzs, jns = _sample_buffers(c, c.x0, ts, jump_to, seeds, sid0)
        assert torch.equal(y, _chain_rs(c, c.x0, ts, jump_to, aux=aux_, keep=keep, noise=nzs, jnoise=jns))
        return y[pos], nzs[:, pos], jns[:, pos]

    y1, nz1, jn1 = run(1, 0, False)
    for B_, pos, aux_ in ((3, 2, False), (16, pos16, True)):
        y, nz, jn = run(B_, pos, aux_)
        assert torch.equal(nz, nz1) and torch.equal(jn, jn1)                    # the noise: bit-equal
        # the images: another batch size may take other convolution kernels, so the bound is the one test_gpu_seeds applies
        # across batch sizes (test_batch_size_does_not_matter: rel-L2 <= BUDGET), not the same-kernel bound
        err = rel_l2(y.cpu(), y1.cpu())
        print(f"seeded sample at position {pos} of {B_} (two streams={aux_}) vs batch of one: rel-L2 {err:.3e} (budget "
              f"{BUDGET:.0e}) max-abs {max_abs(y.cpu(), y1.cpu()):.3e} bit-equal {torch.equal(y, y1)}")
        assert err <= BUDGET


# ---- 8: the marginal ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,l2", [(200, 201), (200, 209), (21, 30)], ids=["J2", "J10", "J10_low"])
def test_step_and_jump_land_on_the_marginal(t, l2):
    """Mask == 1, mode 1, one step + jump with in-kernel noise on 67x90 at batch 2 (36 180 elements).  Under a full mask the
    result does not depend on the network, and (out - sa[l2] M_l2) / sb[l2] with x0 = k0 is N(0,1): |mean| <= 5 / sqrt(N),
    |variance - 1| <= 5 sqrt(2 / N).  A jump that reused the step's draw would miss the variance (the restatement shows by
    how much: tests/test_resample_host.py)."""
    c = _ctx("C2", 160, 1, 2, 0)
    c.d.omega = 0.0                                                             # (the configs' own setting)
    B, N = 2, 2 * 3 * c.H * c.W
    assert N >= 36000 and c.d._coef_table(1)[t].mode == 1
    ones = torch.ones_like(c.m)
    y = _chain_rs(c, c.x0, [t], [l2], seed=31337, sid0=(1 << 32) | 2, keep=(ones, c.k0))
    other = _chain_rs(c, (c.x0 * 0.3 + 0.1).contiguous(), [t], [l2], seed=31337, sid0=(1 << 32) | 2, keep=(ones, c.k0))
    assert torch.equal(y, other)                                                # the network does not matter
    wz = whitened(y, c.d, 1, l2, c.xt, c.k0[None].expand(B, -1, -1, -1))
    mean, var = float(wz.mean()), float(wz.var(unbiased=False))
    lim_m, lim_v = moment_limits(N)
    print(f"t={t} -> level {l2}: N={N} whitened mean {mean:+.5f} (limit {lim_m:.5f}) variance {var:.5f} (1 +- {lim_v:.5f})")
    assert abs(mean) <= lim_m and abs(var - 1.0) <= lim_v


# ---- 9: the public mode ------------------------------------------------------------------------------------------------------
def test_inpaint_with_resampling_on_c1(golden, tmp_path):
    from sinddm_amd.functions import keep_mask_pyramid
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    sizes = [tuple(s) for s in meta["image_sizes_hw"]]
    H, W = sizes[-1]
    mask = torch.ones(H, W)
    mask[31:61, 43:83] = 0                                                      # a 30x40 hole
    seeds, tl = [11, 12], em.num_timesteps_ideal[1:]
    em.draw_log = []
    outs = tr.inpaint(mask, batch_size=2, custom_t_list=tl, save_images=False, seeds=seeds, resample=2, jump_length=2)
    log, em.draw_log = em.draw_log, None
    assert em.resample is None and em.keep_maps is None
    assert [e[0] for e in log] == ["init", "chain_resample", "renoise", "chain_resample", "renoise", "chain_resample"]
    for e in (e for e in log if e[0] == "chain_resample"):
        _, s, sd, steps, jump_to = e
        plain = sorted(set(steps), reverse=True)
        assert sd == seeds and len(steps) == len(jump_to) == closed_form_count(plain, 2, 2) > len(plain)
        print(f"scale {s}: {len(plain)} plain steps, {len(steps)} evaluations with R = 2, J = 2")
    masks = keep_mask_pyramid(mask, sizes, hard=True)
    for s in range(len(sizes)):
        kept = masks[s].bool().to(DEV)
        img = tr.data_list[s][0][0]
        assert torch.isfinite(outs[s]).all()
        assert torch.equal(outs[s][:, :, kept], img[None].expand(2, -1, -1, -1)[:, :, kept])    # the kept pixels, exactly
    hole = ~mask.bool().to(DEV)
    diff = max_abs(outs[-1][0][:, hole].cpu(), outs[-1][1][:, hole].cpu())
    print(f"inpaint C1 dim 32 T=20 B=2, R=2 J=2: the two samples differ inside the hole by max-abs {diff:.3e}")
    assert diff > 1e-2
    # resample = 1 is the run without jumps: same entries, same images
    em.draw_log = []
    plain = tr.inpaint(mask, batch_size=2, custom_t_list=tl, save_images=False, seeds=seeds)
    log0, em.draw_log = em.draw_log, []
    one = tr.inpaint(mask, batch_size=2, custom_t_list=tl, save_images=False, seeds=seeds, resample=1, jump_length=2)
    log1, em.draw_log = em.draw_log, None
    assert [e[0] for e in log0] == [e[0] for e in log1] == ["init", "chain_seeds", "renoise", "chain_seeds", "renoise", "chain_seeds"]
    assert all(torch.equal(a, b) for a, b in zip(plain, one))
    assert max_abs(plain[-1][:, :, hole].cpu(), outs[-1][:, :, hole].cpu()) > 1e-2      # the jumps moved the hole
    # an error inside the run puts the setting back
    with pytest.raises(ValueError):
        tr.inpaint(mask, batch_size=2, custom_t_list=tl, save_images=False, seeds=[1], resample=2, jump_length=2)
    assert em.resample is None and em.keep_maps is None
    with pytest.raises(ValueError):
        tr.inpaint(mask, batch_size=2, save_images=False, resample=0)
    outs = tr.outpaint((1, 1.5), batch_size=2, custom_t_list=tl, save_images=False, seeds=seeds, resample=2, jump_length=3)
    assert em.resample is None and all(torch.isfinite(o).all() for o in outs)
