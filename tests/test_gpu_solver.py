"""Few-step sampling on the GPU: strided steps through the chain call and the second-order multistep step
(sinddm_sample_chain_solver / sinddm_reverse_step_ms).  With the solver block every step of a call runs unfused -- the
network writes eps -- and ends in ONE elementwise kernel that extrapolates the noise estimate from the previous step's clean
estimate (`hist`) and then evaluates the ordinary step.

The reference has no counterpart, so the yardsticks are a float64 restatement of the formulas (tests/solver_util.py), the
project's own step-by-step route, bit-level identities and the order of accuracy on a problem with a known solution:
  1. sinddm_reverse_step_ms against the float64 restatement (modes 0 / 1, keep and edit off / on, 5x7 and 8x12: 3 H W % 4
     == 1 and == 0, B = 2 so that a quad crosses a sample's end); `hist`; q = 0 is the plain step bit for bit;
  2. the chain equals the same schedule driven step by step, on the five shapes of test_gpu_keep.CASES (one per tail kernel /
     row layout, two streams, tiled) and the 18-sample run whose second half starts inside a quad; on the same shapes, maps
     with a slice per sample equal the shared-map run sample by sample, bit for bit;
  3. identities, bit for bit: Philox == buffers (unseeded, seeded), a run repeats, two streams == one, options at their
     defaults == options unset, so = NULL == sinddm_sample_chain_batch;
  4. the seeds contract through a multistep chain;
  5. the order conditions of tests/test_solver_host.py through the real kernel, (1, 3, 37, 37): 4107 elements, odd, two blocks;
  6. `sample_scales` with sample_steps = 8, order 2 on the C1 pyramid; the combinations that are not built raise.
Four evaluations per chain: levels [T, T // 2, T // 8, 0], the last landing on the clean image.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import max_abs
from sinddm_amd.functions import stride_schedule
from sinddm_amd.synth import hash_randn
from solver_util import Gaussian, kappa, rms, run_ref, solver_q, step_to_ref
from test_gpu_chain_guided import _trainer
from test_gpu_keep import CASE_IDS, CASES, _bound, _draw
from test_gpu_resample import UNALIGNED
from test_gpu_seeds import _ctx, _dev_seeds, _seed_list
from test_solver_host import gaussian_problem, order_conditions

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _sched(T):
    """The four-evaluation schedule of a shape whose walk starts at level T: (taus, lands)."""
    taus = [T, T // 2, T // 8, 0]
    return taus, taus[1:] + [-1]


MS_CASES = [(cfg, dim, s, B, aux, ts[0], hx) for cfg, dim, s, B, aux, ts, hx in CASES]
MS_UNALIGNED = UNALIGNED[:5] + (400, 0)                         # 67x90, 18 samples, two streams: 9 * 3 * 67 * 90 % 4 == 2


def _seeded_draws(c, x0, seeds, n_steps, sid0):
    """What the in-kernel streams give a SEEDED run, as the step-major buffer opts->noise takes: sample b of step i is
    sinddm_normal_fill(3 H W, seeds[b], sid0 + i) over the extended sample."""
    from sinddm_amd import _lib
    lib = _lib.load()
    B, Cc, H, W = x0.shape
    sd = _dev_seeds(seeds)
    out = torch.empty((n_steps, B, Cc, H, W + 2 * c.hx), device=DEV)
    for i in range(n_steps):
        _lib.check(lib.sinddm_normal_fill_samples(_lib.ptr(out[i]), B, out[i].numel() // B, _lib.ptr(sd), sid0 + i,
                                                  _lib.stream_ptr(DEV)), "sinddm_normal_fill_samples")
    return out


def _chain_solver(c, x0, taus, lands, order=2, seed=0, sid0=0, aux=False, edit=None, keep=None, noise=None, seeds=None,
                  entry="solver", so="block", hist=None, q=None, expect_rc=0, per_sample=False):
    """sinddm_sample_chain_solver (or _batch) on centre-size arguments of a test_gpu_keep._Ctx, extended here; the extended
    result.  so: "block" (q of `order`: all zeros for order 1), "null" (so = NULL) or "no_q" (a block whose q is NULL).
    per_sample: the edit and keep maps have a leading batch dimension, one slice per sample (sinddm_batch_opts)."""
    from sinddm_amd import _lib
    from sinddm_amd.models import _aux_stream, _workspace
    lib = _lib.load()
    xa = c.ext(x0).clone()
    B, _, H, We = xa.shape
    n = len(taus)
    xb, eps, xt = torch.empty_like(xa), torch.empty_like(xa), c.ext(c.xt)
    coefs = (_lib.StepCoefs * n)(*[c.d.step_coefs_to(t, u, c.s) for t, u in zip(taus, lands)])
    tl = (C.c_int * n)(*taus)
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
        ab = (C.c_float * (2 * n))(*[float(v) for u in lands for v in ab_tab[u + 1]])
        kopts = _lib.KeepOpts()
        kopts.mask, kopts.x0, kopts.ab = _lib.ptr(held[-2]), _lib.ptr(held[-1]), C.cast(ab, C.POINTER(C.c_float))
    sd = _dev_seeds(seeds) if seeds is not None else None
    args = [_lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
            coefs, tl, n, float(c.s), seed, sid0, c.dim, B, H, We - 2 * c.hx, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
            _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, c.hx,
            C.byref(kopts) if kopts is not None else None, _lib.ptr(sd), None, None,
            C.byref(_lib.BatchOpts(int(edit is not None), int(keep is not None), int(keep is not None), 0, None)) if per_sample else None]
    if entry == "batch":
        rc = lib.sinddm_sample_chain_batch(*args)
    else:
        if q is None:
            q = c.d._solver_q(c.s, taus, lands) if order == 2 else [0.0] * n
        qarr = (C.c_float * n)(*q)
        hist = torch.full_like(xa, float("nan")) if hist is None else hist      # (a step reads it only after one has written it)
        sopts = _lib.SolverOpts(None if so == "no_q" else C.cast(qarr, C.POINTER(C.c_float)), _lib.ptr(hist))
        rc = lib.sinddm_sample_chain_solver(*args, None if so == "null" else C.byref(sopts))
    torch.cuda.synchronize()
    assert rc == expect_rc
    if rc != 0:
        return None
    assert flag.value in (0, 1)
    return xb if flag.value == 1 else xa


def _stepwise(c, taus, lands, order, nz, edit=False, keep=False):
    """The same schedule through `_p_sample_host_t`, fed the centre of the draws `nz`."""
    d = c.d
    d.roi_guided_sampling = edit
    d.keep_maps = {c.s: (c.m, c.k0)} if keep else None
    q = d._solver_q(c.s, taus, lands) if order == 2 else None
    x = c.x0.clone()
    hist = torch.full_like(x, float("nan")) if order == 2 else None
    for i, (t, u) in enumerate(zip(taus, lands)):
        d.noise_fn = lambda kind, shape, ss, tt, dev, z=c.centre(nz[i]): z
        x = d._p_sample_host_t(x, t, c.s, step_pos=i, land=u, q=q[i] if q else None, hist=hist)
    d.noise_fn, d.keep_maps, d.roi_guided_sampling = None, None, False
    return x


# ---- 1: the stepwise kernel against the float64 restatement ------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (8, 12)], ids=["5x7", "8x12"])
@pytest.mark.parametrize("s,prev,t,u", [(0, 900, 700, 400), (1, 350, 200, 50)], ids=["mode0", "mode1"])
def test_reverse_step_ms_against_float64(s, prev, t, u, H, W):
    from sinddm_amd import _lib
    from sinddm_amd.configs import build_diffusion
    lib = _lib.load()
    net, d = build_diffusion("C2", dim=20, device=DEV)
    d.omega = 0.3                                                               # (a step sigma that shows: see test_gpu_seeds._ctx)
    B = 2
    assert (3 * H * W) % 4 == (1 if (H, W) == (5, 7) else 0)
    x, eps, xt, z, hist0 = ((hash_randn((B, 3, H, W), 250 + i) * a).to(DEV) for i, a in enumerate((0.8, 1.0, 0.5, 1.0, 0.6)))
    m = torch.zeros(H, W)
    m[1:4, 2:6] = 1
    m[3:, 4:] = 0.25
    m, k0 = m.to(DEV), (hash_randn((3, H, W), 271) * 0.6).clamp(-1, 1).to(DEV)
    ew = (0.2 + 0.8 * hash_randn((H, W), 260).abs().clamp(0, 1)).to(DEV)
    ec = (hash_randn((3, H, W), 261) * 0.3).to(DEV)
    k = d.step_coefs_to(t, u, s)
    assert k.mode == (0 if s == 0 else 1)
    q = float(np.float32(d._solver_q(s, [prev, t], [t, u])[1]))                # (what the kernel gets: one fp32 scalar)
    assert q == float(np.float32(solver_q(d, s, [prev, t], [t, u])[1])) and 0.1 < q < 10.0
    ka, kb = (float(v) for v in d._keep_ab_table()[u + 1])
    st = _lib.stream_ptr(DEV)
    xt_arg = xt if s > 0 else None
    xp_ref = step_to_ref(d, s, t, u, x, eps, xt_arg, z)[1]
    for keep in (False, True):
        for edit in (False, True):
            kw = dict(edit=(ew, ec) if edit else None, keep=(m, k0) if keep else None)
            ref, _ = step_to_ref(d, s, t, u, x, eps, xt_arg, z, q=q, hist=hist0, **kw)
            bound = 4e-6 * max(1.0, float(ref.abs().max()))
            # first, on the CPU: the restatement evaluated in fp32 stays within half the bound (the bound leaves room)
            ref32, _ = step_to_ref(d, s, t, u, x, eps, xt_arg, z, q=q, hist=hist0, dtype=torch.float32, **kw)
            assert ref32.dtype == torch.float32
            err32 = float((ref32.double() - ref).abs().max())
            assert err32 <= 0.5 * bound, (err32, bound)
            guard = 7.5
            buf = torch.full((x.numel() + 8,), guard, device=DEV)               # (the last quad must not write past the end)
            hbuf = torch.full((x.numel() + 8,), guard, device=DEV)
            hbuf[:x.numel()] = hist0.reshape(-1)
            args = lambda out, qq, hh: (_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt_arg), _lib.ptr(z), _lib.ptr(out), C.byref(k), qq,
                                        _lib.ptr(hh), _lib.ptr(ew) if edit else None, _lib.ptr(ec) if edit else None,
                                        _lib.ptr(m) if keep else None, _lib.ptr(k0) if keep else None, ka, kb, B, 3, H * W, st)
            rc = lib.sinddm_reverse_step_ms(*args(buf, q, hbuf))
            torch.cuda.synchronize()
            assert rc == 0
            assert bool((buf[x.numel():] == guard).all()) and bool((hbuf[x.numel():] == guard).all())
            out, hist = buf[:x.numel()].view_as(x), hbuf[:x.numel()].view_as(x)
            err = float((out.cpu().double() - ref).abs().max())
            herr, hbound = float((hist.cpu().double() - xp_ref).abs().max()), 4e-6 * max(1.0, float(xp_ref.abs().max()))
            print(f"s={s} {prev} > {t} -> {u} q={q:.4f} {H}x{W} keep={keep} edit={edit}: reverse_step_ms vs float64 max-abs "
                  f"{err:.3e} (bound {bound:.3e}; restatement in fp32 {err32:.3e}); hist vs xp {herr:.3e} (bound {hbound:.3e})")
            assert err <= bound and herr <= hbound
            # the extrapolation is not a no-op: the first-order step lands elsewhere
            plain_ref, _ = step_to_ref(d, s, t, u, x, eps, xt_arg, z, **kw)
            assert float((plain_ref - ref).abs().max()) > 1e-2
            # q = 0 is the plain step, bit for bit, and reads no history
            out0, h0 = torch.empty_like(x), torch.full_like(x, float("nan"))
            assert lib.sinddm_reverse_step_ms(*args(out0, 0.0, h0)) == 0
            plain = torch.empty_like(x)
            if keep:
                rc = lib.sinddm_reverse_step_keep(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt_arg), _lib.ptr(z), _lib.ptr(plain), C.byref(k),
                                                  _lib.ptr(ew) if edit else None, _lib.ptr(ec) if edit else None, _lib.ptr(m),
                                                  _lib.ptr(k0), ka, kb, B, 3, H * W, st)
            elif edit:
                rc = lib.sinddm_reverse_step_edit(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt_arg), _lib.ptr(z), _lib.ptr(plain), C.byref(k),
                                                  _lib.ptr(ew), _lib.ptr(ec), B, 3, H * W, st)
            else:
                rc = lib.sinddm_reverse_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt_arg), _lib.ptr(z), _lib.ptr(plain), C.byref(k),
                                             x.numel(), st)
            torch.cuda.synchronize()
            assert rc == 0
            print(f"    q = 0 vs the plain step: max-abs {max_abs(out0.cpu(), plain.cpu()):.3e} bit-equal {torch.equal(out0, plain)}")
            assert torch.equal(out0, plain)
            assert torch.isfinite(h0).all() and float((h0.cpu().double() - xp_ref).abs().max()) <= hbound
    # the multistep factor on a mode-2 step does not exist
    k2 = d.step_coefs_to(t, -1, 1)
    assert k2.mode == 2
    out, h = torch.empty_like(x), torch.zeros_like(x)
    call2 = lambda qq: lib.sinddm_reverse_step_ms(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(out), C.byref(k2), qq,
                                                  _lib.ptr(h), None, None, None, None, 1.0, 0.0, B, 3, H * W, st)
    assert call2(0.5) == -1 and call2(0.0) == 0
    torch.cuda.synchronize()


# ---- 2: chain equals stepwise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "maps", "recorded", "per_sample_maps"])
@pytest.mark.parametrize("cfg,dim,s,B,aux,T,hx", MS_CASES + [MS_UNALIGNED], ids=CASE_IDS + ["pitch_67x90_B18_unaligned_half"])
def test_multistep_chain_equals_stepwise(cfg, dim, s, B, aux, T, hx, variant):
    c = _ctx(cfg, dim, s, B, hx)
    seed = 818181 + s
    taus, lands = _sched(T)
    assert c.d.step_coefs_to(taus[-1], -1, s).mode == (0 if s == 0 else 2)
    if variant == "per_sample_maps":
        # Maps with a slice per sample: where 3 H W % 4 != 0 (67x90, 133x177) a quad of the unseeded launch runs over a sample's
        # end into the next sample's slices.  The stride is address arithmetic only, so the yardstick is the shared-map run
        # of the lines below: sample b of the run on row b's maps, bit for bit (first, second and last sample).
        from test_gpu_batch_maps import _maps
        mp = _maps(c, B)
        y = _chain_solver(c, c.x0, taus, lands, seed=seed, aux=aux, edit=(mp["ew"], mp["ec"]), keep=(mp["m"], mp["k0"]), per_sample=True)
        assert torch.isfinite(y).all()
        for b in sorted({0, 1, B - 1}):
            row = {k: v[b].clone() for k, v in mp.items()}                  # (a tensor of its own: the entry wants 16-byte aligned maps)
            yb = _chain_solver(c, c.x0, taus, lands, seed=seed, aux=aux, edit=(row["ew"], row["ec"]), keep=(row["m"], row["k0"]))
            assert torch.equal(y[b], yb[b]), b
            assert not torch.equal(y[(b + 1) % B], yb[(b + 1) % B])         # (the rows differ, and it shows)
        return
    maps = variant == "maps"
    kw = dict(edit=(c.ew, c.ec), keep=(c.m, c.k0)) if maps else {}
    nz = torch.stack([_draw(c, c.x0, seed, i) for i in range(len(taus))]).contiguous()
    x = _stepwise(c, taus, lands, 2, nz, edit=maps, keep=maps)
    if variant == "recorded":
        y = _chain_solver(c, c.x0, taus, lands, aux=aux, noise=nz, **kw)
    else:
        y = _chain_solver(c, c.x0, taus, lands, seed=seed, aux=aux, **kw)
    assert torch.isfinite(y).all()
    err, bound = max_abs(c.centre(y).cpu(), x.cpu()), _bound(x)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B} {variant}: multistep chain vs stepwise max-abs {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound
    # the second order is at work: the same schedule at first order lands elsewhere
    y1 = _chain_solver(c, c.x0, taus, lands, order=1, seed=seed, aux=aux, noise=nz if variant == "recorded" else None, **kw)
    assert max_abs(y1.cpu(), y.cpu()) > 1e-3
    if variant == "plain":
        # ... and first order through the block is the strided chain without it, to the bound (fused tails there)
        y1b = _chain_solver(c, c.x0, taus, lands, seed=seed, aux=aux, entry="batch")
        assert max_abs(c.centre(y1b).cpu(), c.centre(y1).cpu()) <= _bound(y1)
        x1 = _stepwise(c, taus, lands, 1, nz)
        assert max_abs(c.centre(y1b).cpu(), x1.cpu()) <= _bound(x1)


# ---- 3: identities, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,T,hx", MS_CASES + [MS_UNALIGNED], ids=CASE_IDS + ["pitch_67x90_B18_unaligned_half"])
def test_multistep_identities(cfg, dim, s, B, aux, T, hx):
    c = _ctx(cfg, dim, s, B, hx)
    keep = (c.m, c.k0)
    seed, sid0 = 787 + s, (s << 32) | 2
    taus, lands = _sched(T)
    y0 = _chain_solver(c, c.x0, taus, lands, seed=seed, sid0=sid0, aux=aux, keep=keep)
    assert torch.isfinite(y0).all()
    assert torch.equal(y0, _chain_solver(c, c.x0, taus, lands, seed=seed, sid0=sid0, aux=aux, keep=keep))         # repeats
    if aux:
        assert torch.equal(y0, _chain_solver(c, c.x0, taus, lands, seed=seed, sid0=sid0, aux=False, keep=keep))   # one stream
    nz = torch.stack([_draw(c, c.x0, seed, sid0 + i) for i in range(len(taus))]).contiguous()
    y1 = _chain_solver(c, c.x0, taus, lands, aux=aux, keep=keep, noise=nz)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B}: Philox vs buffers max-abs {max_abs(y0.cpu(), y1.cpu()):.3e} "
          f"bit-equal {torch.equal(y0, y1)}")
    assert torch.equal(y0, y1)
    seeds = _seed_list(B)
    ys = _chain_solver(c, c.x0, taus, lands, seed=999, sid0=sid0, aux=aux, keep=keep, seeds=seeds)               # (`seed` is ignored)
    if aux:
        assert torch.equal(ys, _chain_solver(c, c.x0, taus, lands, sid0=sid0, aux=False, keep=keep, seeds=seeds))
    nzs = _seeded_draws(c, c.x0, seeds, len(taus), sid0)
    ys1 = _chain_solver(c, c.x0, taus, lands, aux=aux, keep=keep, noise=nzs)
    print(f"    seeded: max-abs {max_abs(ys.cpu(), ys1.cpu()):.3e} bit-equal {torch.equal(ys, ys1)}")
    assert torch.equal(ys, ys1)
    assert max_abs(ys.cpu(), y0.cpu()) > 1e-2
    # a run cut into two calls continues: the history survives between them
    hist = torch.full_like(c.ext(c.x0), float("nan"))
    q = c.d._solver_q(s, taus, lands)
    ya = _chain_solver(c, c.x0, taus[:2], lands[:2], seed=seed, sid0=sid0, aux=aux, keep=keep, hist=hist, q=q[:2])
    assert torch.isfinite(c.centre(hist)).all()
    yb = _chain_solver(c, c.centre(ya), taus[2:], lands[2:], seed=seed, sid0=sid0 + 2, aux=aux, keep=keep, hist=hist, q=q[2:])
    assert torch.equal(c.centre(yb), c.centre(y0))
    # so = NULL, or a block without q, is sinddm_sample_chain_batch itself
    ref = _chain_solver(c, c.x0, taus, lands, seed=seed, sid0=sid0, aux=aux, keep=keep, entry="batch")
    for so in ("null", "no_q"):
        assert torch.equal(ref, _chain_solver(c, c.x0, taus, lands, seed=seed, sid0=sid0, aux=aux, keep=keep, so=so)), so


@pytest.mark.parametrize("idx", [0, 1, 3], ids=[CASE_IDS[i] for i in (0, 1, 3)])
def test_default_options_are_the_run_without_them(idx):
    """`_run_steps` with sample_steps >= len(t_seq), order 1 and eta = 1 goes through the strided scalars and computes what
    the run with the options unset computes, bit for bit; the log entry is the same."""
    cfg, dim, s, B, aux, T, hx = MS_CASES[idx]
    c = _ctx(cfg, dim, s, B, hx)
    d = c.d
    d.two_streams = aux
    run = [T, T - 1, T - 2]
    outs, logs = [], []
    for steps in (None, 3, 50):
        d.sample_steps = steps
        torch.manual_seed(77)
        d.draw_log = []
        outs.append(d._run_steps(c.x0.clone(), s, run))
        logs.append(d.draw_log)
        d.draw_log = None
    d.sample_steps = None
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert logs[0] == logs[1] == logs[2] and logs[0][0][3] == run
    # ... and fewer steps is another run, logged with the levels it evaluated
    d.sample_steps, d.draw_log = 2, []
    torch.manual_seed(77)
    y2 = d._run_steps(c.x0.clone(), s, run)
    log, d.draw_log, d.sample_steps = d.draw_log, None, None
    assert log[0][3] == [T, T - 2] and not torch.equal(y2, outs[0])
    # `_run_steps` at order 2 is the direct call with the seed it drew
    taus, lands = stride_schedule(list(range(T, -1, -1)), 4, "t")
    d.sample_steps, d.solver_order, d.draw_log = 4, 2, []
    torch.manual_seed(78)
    y_api = d._run_steps(c.x0.clone(), s, range(T, -1, -1))
    log, d.draw_log, d.sample_steps, d.solver_order = d.draw_log, None, None, 1
    assert log[0][3] == taus
    assert torch.equal(y_api, c.centre(_chain_solver(c, c.x0, taus, lands, seed=log[0][2], aux=aux)))


# ---- 4: the seeds contract ---------------------------------------------------------------------------------------------------
def test_seeded_sample_through_a_multistep_chain_at_any_position():
    """Sample b of a B = 4 run equals the B = 1 run of its seed.  The bound is the same-kernel bound, so the shape must be one
    whose convolutions take the same kernels at both batch sizes: the first of the candidates below for which the library
    says so (sinddm_debug_routes)."""
    from sinddm_amd import _lib
    lib = _lib.load()

    def routes(dim, B, H, W):
        out = (C.c_int * 16)()
        assert lib.sinddm_debug_routes(dim, 0, B, H, W, out) == 0
        return list(out)

    pick = None
    for cfg, dim, s, T in (("C2", 20, 3, 311), ("C2", 160, 0, 700)):
        c4 = _ctx(cfg, dim, s, 4, 0)
        if routes(dim, 1, c4.H, c4.W) == routes(dim, 4, c4.H, c4.W):
            pick = (cfg, dim, s, T, c4)
            break
    assert pick is not None
    cfg, dim, s, T, c4 = pick
    taus, lands = _sched(T)
    sid0, seeds = (s << 32) | 2, [1000 + 17 * b for b in range(4)]
    y4 = _chain_solver(c4, c4.x0, taus, lands, sid0=sid0, seeds=seeds)
    for b in (0, 2, 3):
        c1 = _ctx(cfg, dim, s, 1, 0)
        c1.x0, c1.xt = c4.x0[b:b + 1].clone(), None if c4.xt is None else c4.xt[b:b + 1].clone()
        y1 = _chain_solver(c1, c1.x0, taus, lands, sid0=sid0, seeds=[seeds[b]])
        err, bound = max_abs(y4[b:b + 1].cpu(), y1.cpu()), _bound(y1)
        print(f"{cfg} dim {dim} s={s} {c4.H}x{c4.W}: seeded sample {b} of 4 vs batch of one max-abs {err:.3e} (bound {bound:.3e}) "
              f"bit-equal {torch.equal(y4[b:b + 1], y1)}")
        assert err <= bound
    assert max_abs(y4[0].cpu(), y4[1].cpu()) > 1e-2


# ---- 5: the order of accuracy, through the real kernel -------------------------------------------------------------------------
def test_order_on_the_analytic_gaussian_through_the_kernel():
    from sinddm_amd import _lib
    from sinddm_amd.configs import build_diffusion
    lib = _lib.load()
    net, d = build_diffusion("C2", dim=20, device=DEV)
    assert d.omega == 0
    shape = (1, 3, 37, 37)
    G, x64, xt64, exact = gaussian_problem(d, n=3 * 37 * 37, shape=shape)
    run, kap = list(range(311, -1, -1)), kappa(d, 3)
    st = _lib.stream_ptr(DEV)
    xt, zero = xt64.float().to(DEV), torch.zeros(shape, device=DEV)

    def gpu_run(taus, lands, order):
        q = d._solver_q(3, taus, lands) if order == 2 else [0.0] * len(taus)
        x, out, hist = x64.float().to(DEV), torch.empty(shape, device=DEV), torch.full(shape, float("nan"), device=DEV)
        for i, (t, u) in enumerate(zip(taus, lands)):
            eps = G.eps(x, t).contiguous()                                      # the analytic denoiser, in torch on the device
            k = d.step_coefs_to(t, u, 3, clip_denoised=False)
            rc = lib.sinddm_reverse_step_ms(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(zero), _lib.ptr(out), C.byref(k), q[i],
                                            _lib.ptr(hist), None, None, None, None, 1.0, 0.0, 1, 3, 37 * 37, st)
            assert rc == 0
            x, out = out, x
        torch.cuda.synchronize()
        return x.cpu().double()

    e, floor = {1: {}, 2: {}}, 0.0
    for order in (1, 2):
        for n in (20, 40):
            taus, lands = stride_schedule(run, n, "t")
            e[order][n] = rms(gpu_run(taus, lands, order), exact)
            if order == 2:
                floor = max(floor, rms(run_ref(d, 3, taus, lands, x64, G.eps, 2, x_tilde=xt64, round32=True),
                                       run_ref(d, 3, taus, lands, x64, G.eps, 2, x_tilde=xt64)))
    taus, lands = stride_schedule(run, 10, "logsnr", kap)
    e2_log = rms(gpu_run(taus, lands, 2), exact)
    floor = max(floor, rms(run_ref(d, 3, taus, lands, x64, G.eps, 2, x_tilde=xt64, round32=True),
                           run_ref(d, 3, taus, lands, x64, G.eps, 2, x_tilde=xt64)))
    print(f"fp32 floor of the e2 values (float64 restatement rounded to fp32 after every step vs not): {floor:.3e}")
    assert floor < 1e-4
    order_conditions(e[1], e[2], e2_log, slack=floor)


# ---- 6: the public mode ------------------------------------------------------------------------------------------------------
def test_few_step_sample_scales_on_c1(golden, tmp_path):
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    sizes = [tuple(s) for s in meta["image_sizes_hw"]]
    tl = em.num_timesteps_ideal[1:]
    lens = [em.num_timesteps] + list(tl)
    try:
        for spacing in ("logsnr", "t"):
            em.sample_steps, em.solver_order, em.sample_spacing, em.draw_log = 8, 2, spacing, []
            torch.manual_seed(97)
            outs = tr.sample_scales(batch_size=2, custom_t_list=tl, save_images=False)
            log, em.draw_log = em.draw_log, None
            assert [tuple(o.shape) for o in outs] == [(2, 3) + hw for hw in sizes]
            assert all(torch.isfinite(o).all() for o in outs)
            chains = [e for e in log if e[0] == "chain"]
            assert [e[0] for e in log] == ["init", "chain", "renoise", "chain", "renoise", "chain"]
            for e, n in zip(chains, lens):
                want = stride_schedule(list(range(n - 1, -1, -1)), 8, spacing, em._kappa(e[1]))[0]
                print(f"{spacing}: scale {e[1]}: {n} levels, evaluated at {e[3]}")
                assert e[3] == want and len(e[3]) <= min(8, n) and e[3][0] == n - 1 and e[3][-1] == 0
                if spacing == "t":
                    assert len(e[3]) == min(8, n)                               # ('logsnr' may name a level twice and drop it)
        plain = tr.sample_scales(batch_size=2, custom_t_list=tl, save_images=False)
        # the combinations that are not built
        img = outs[0]
        em.sample_steps, em.solver_order, em.sample_spacing = 8, 1, "t"
        em.resample = (2, 2)
        with pytest.raises(NotImplementedError):
            em._run_steps(img, 0, range(19, -1, -1))
        em.resample = None
        em.solver_order = 2
        em.layout_maps, em.layout_down = {0: torch.zeros((3,) + sizes[0], device=DEV)}, {0: 4}
        with pytest.raises(NotImplementedError):
            em._run_steps(img, 0, range(19, -1, -1))
        em.solver_order = 1                                                     # (first order does combine with a layout)
        assert torch.isfinite(em._run_steps(img, 0, range(19, -1, -1))).all()
        em.layout_maps, em.layout_down = None, {}
        for name, val in (("sample_steps", 8), ("solver_order", 2), ("eta", 0.5)):
            em.sample_steps, em.solver_order, em.eta = None, 1, 1.0
            setattr(em, name, val)
            em.clip_guided_sampling = True
            with pytest.raises(NotImplementedError):
                em._run_steps(img, 0, range(19, -1, -1))
            em.clip_guided_sampling = False
        # eta = 0 makes scale 0 deterministic: two runs from one start agree whatever the draws
        em.sample_steps, em.solver_order, em.eta = 8, 1, 0.0
        a, b = em._run_steps(img, 0, range(19, -1, -1)), em._run_steps(img, 0, range(19, -1, -1))
        assert torch.equal(a, b)
        em.eta = 1.0
        assert not torch.equal(em._run_steps(img, 0, range(19, -1, -1)), em._run_steps(img, 0, range(19, -1, -1)))
    finally:
        em.sample_steps, em.solver_order, em.sample_spacing, em.eta, em.resample, em.layout_maps = None, 1, "t", 1.0, None, None
        em.clip_guided_sampling, em.draw_log = False, None
    assert all(torch.isfinite(o).all() for o in plain)
