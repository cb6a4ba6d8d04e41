"""Per-pixel edit strength: the known-region keep gated by level inside the sampler chain (sinddm_sample_chain_gate /
sinddm_reverse_step_keep_gate).  The mask plane is a hold level h(p); step i keeps the pixels with h(p) >= thr[i], fully, and
leaves the rest to the model -- each pixel its own SDEdit start level.

The reference has no counterpart, so the yardsticks are exactness properties and the project's own step-by-step route:
  G1. the gated chain equals the step-by-step route (sinddm_net_forward + sinddm_reverse_step_keep_gate) on every tail kernel,
      with and without ROI edit maps; `_run_steps` is the direct call with the thresholds of functions.gate_thresholds;
  G2. the gate changes no arithmetic: one-step gated calls are bit-equal to ungated sinddm_sample_chain_keep calls whose masks
      are (h >= thr_i) built in torch -- and the gated run is neither the (h > 0) run nor the run without keep;
  G3. invisible ends: a binary hold map with any thresholds is sinddm_sample_chain_keep, gt = NULL is sinddm_sample_chain_mix;
  G4. exact pixels: h = 1 down to t = 0 is the known image; after one step h < thr is the plain call's pixel bit for bit and
      h >= thr is keep_a * target + keep_b * z of the same z;
  G5. composition: one and two streams, a noise buffer of the Philox numbers, per-sample hold maps on both sides of the
      two-stream split, and a gated run through the jump, multistep and layout tails against the step-by-step entries;
  G6. sinddm_reverse_step_keep_gate against the blend assembled in torch, modes 0, 1, 2, thr below / at / above a plateau;
  G7. `MultiscaleTrainer.edit` on the C1 pyramid.
Shapes: the four of test_gpu_chain_guided.SHAPES (each reaches one tail kernel; three steps incl. t = 0) and the tiled case of
test_gpu_keep.  Hold map: plateaus at exactly 0, 0.25, 0.5, 0.6 and 1, edges off the quad grid, contact with two borders.
Thresholds [0.2, 0.5, 1.0]: every step keeps another set of plateaus, and h == thr occurs at 0.5 and at 1.0 (kept).
Where a tolerance is needed it is `_bound` of test_gpu_keep: 4e-6 * max(1, |ref|max)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import max_abs
from sinddm_amd.functions import gate_thresholds, hold_pyramid, keep_mask_pyramid
from sinddm_amd.synth import hash_randn
from test_gpu_chain_guided import _fill, _trainer
from test_gpu_keep import CASE_IDS, CASES, _bound, _Ctx, _draw, _known

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
THR = [0.2, 0.5, 1.0]
LEVELS = (0.0, 0.25, 0.5, 0.6, 1.0)


def _hold(H, W, variant=0):
    """The hold map: five plateaus, edges off the quad grid (x = 13, 33, 5; widths 30, 14), contact with the right and the
    bottom border.  `variant` moves the plateaus around (per-sample maps)."""
    h = torch.zeros(H, W)
    h[5:25, 8:32] = 1
    h[14:31, 13:43] = 0.25
    h[3:13, 33:47] = 0.5
    h[27:41, 5:19] = 0.6
    h[H - 11:, W - 9:] = 1
    if variant:
        h = torch.roll(h, shifts=(3 * variant, 5 * variant), dims=(0, 1))
        if variant % 2:
            h = torch.where(h == 0.25, torch.full_like(h, 0.6), torch.where(h == 0.6, torch.full_like(h, 0.25), h))
    assert sorted(set(h.flatten().tolist())) == [float(np.float32(v)) for v in LEVELS]
    return h.to(DEV)


def _gated_mask(h, thr):
    """What the gate hands the step: (h >= thr) as 0 / 1, the compare in fp32."""
    return (h >= torch.tensor(thr, dtype=torch.float32, device=h.device)).to(torch.float32)


def _gchain(c, x0, ts, seed, sid0=0, aux=False, edit=None, noise=None, keep=None, thr=None, entry="gate", per_sample=False,
            gate_null=False):
    """sinddm_sample_chain_gate (or _mix / _keep / _tile) on centre-size arguments, extended here; the extended result.
    keep = (hold or mask, known image): (H, W) or, with `per_sample`, (B, H, W)."""
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
    kopts = None
    if keep is not None:
        held += [c.ext(keep[0]), c.ext(keep[1])]
        ab_tab = c.d._keep_ab_table()
        ab = (C.c_float * (2 * n))(*[float(v) for t in ts for v in ab_tab[t]])
        kopts = _lib.KeepOpts(_lib.ptr(held[-2]), _lib.ptr(held[-1]), C.cast(ab, C.POINTER(C.c_float)))
    bopts = _lib.BatchOpts(0, 1, 0, 0, None) if per_sample else None
    tarr = (C.c_float * n)(*thr) if thr is not None else None
    gopts = _lib.GateOpts(C.cast(tarr, C.POINTER(C.c_float)) if tarr is not None else None)
    ref = lambda o: C.byref(o) if o is not None else None
    args = [_lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
            coefs, tl, n, float(c.s), seed, sid0, c.dim, B, H, We - 2 * c.hx, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
            _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, c.hx]
    if entry == "gate":
        rc = lib.sinddm_sample_chain_gate(*args, ref(kopts), None, None, None, ref(bopts), None, None, None if gate_null else ref(gopts))
    elif entry == "mix":
        assert thr is None
        rc = lib.sinddm_sample_chain_mix(*args, ref(kopts), None, None, None, ref(bopts), None, None)
    elif entry == "keep":
        assert thr is None and not per_sample
        rc = lib.sinddm_sample_chain_keep(*args, ref(kopts))
    else:
        assert thr is None and keep is None and not per_sample
        rc = lib.sinddm_sample_chain_tile(*args)
    torch.cuda.synchronize()
    assert rc == 0 and flag.value in (0, 1)
    return xb if flag.value == 1 else xa


@pytest.fixture(scope="module")
def ctx():
    """One _Ctx per case, built once and shared: the tests only read it (the diffusion's options are put back)."""
    made = {}

    def get(cfg, dim, s, B, hx):
        key = (cfg, dim, s, B, hx)
        if key not in made:
            c = _Ctx(cfg, dim, s, B, hx)
            c.h, c.k0 = _hold(c.H, c.W), _known(c.H, c.W)
            made[key] = c
        return made[key]
    return get


# ---- G1: the gated chain equals the step-by-step route ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_edit", [False, True], ids=["gate", "gate_edit"])
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_gated_chain_equals_stepwise(ctx, cfg, dim, s, B, aux, ts, hx, with_edit):
    from sinddm_amd.sampler import RunPlan
    c = ctx(cfg, dim, s, B, hx)
    d, seed = c.d, 626262 + s
    edit = (c.ew, c.ec) if with_edit else None
    try:
        d.roi_guided_sampling = with_edit
        d.keep_maps, d.keep_gated = {s: (c.h, c.k0)}, True
        # the step-by-step route on the run's plan, its thresholds replaced by the test's
        d.noise_fn = lambda *a: None
        plan = RunPlan(d, c.x0, s, ts)
        assert plan.gated and [st.t for st in plan.steps] == list(ts)
        for st, thr in zip(plan.steps, THR):
            st.thr = float(np.float32(thr))
        x = c.x0.clone()
        for i, st in enumerate(plan.steps):
            z = c.centre(_draw(c, c.x0, seed, i))
            d.noise_fn = lambda kind, shape, ss, tt, dev, z=z: z
            x = d._p_sample_host_t(x, st.t, s, step_pos=st.pos, plan=plan)
        d.noise_fn = None
        y = _gchain(c, c.x0, ts, seed, aux=aux, edit=edit, keep=(c.h, c.k0), thr=THR)
        assert torch.isfinite(y).all()
        err, bound = max_abs(c.centre(y).cpu(), x.cpu()), _bound(x)
        print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B} edit={with_edit}: gated chain vs stepwise max-abs {err:.3e} "
              f"(bound {bound:.3e})")
        assert err <= bound
        # ... and the public route is exactly this call with the seed it drew and the thresholds of the rule
        rule = gate_thresholds([t - 1 for t in ts], ts[0]).tolist()
        torch.manual_seed(11)
        seed_api = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
        torch.manual_seed(11)
        d.two_streams = aux
        d.draw_log = []
        y_api = d._run_steps(c.x0.clone(), s, ts)
        log, d.draw_log = d.draw_log, None
        assert len(log) == 1 and log[0][0] == ("chain_tile" if hx else "chain") and log[0][2] == seed_api      # entries unchanged
        assert torch.equal(y_api, c.centre(_gchain(c, c.x0, ts, seed_api, aux=aux, edit=edit, keep=(c.h, c.k0), thr=rule)))
    finally:
        d.noise_fn, d.draw_log, d.roi_guided_sampling, d.keep_maps, d.keep_gated = None, None, False, None, False


# ---- G2, G3: no new arithmetic, invisible ends --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_gate_changes_no_arithmetic(ctx, cfg, dim, s, B, aux, ts, hx):
    c = ctx(cfg, dim, s, B, hx)
    seed = 434343 + s
    sets = [int(_gated_mask(c.h, thr).sum()) for thr in THR]
    assert sets[0] > sets[1] > sets[2] > 0                                          # each step keeps another set of plateaus
    assert bool((c.h == np.float32(THR[1])).any()) and bool((c.h == np.float32(THR[2])).any())     # h == thr occurs
    x = c.x0
    for i, (t, thr) in enumerate(zip(ts, THR)):
        y = _gchain(c, x, [t], seed, sid0=i, aux=aux, keep=(c.h, c.k0), thr=[thr])
        y_ref = _gchain(c, x, [t], seed, sid0=i, aux=aux, keep=(_gated_mask(c.h, thr), c.k0), entry="keep")
        assert torch.equal(y, y_ref), f"step {i} (t = {t}, thr = {thr})"
        x = c.centre(y)
    # the gate is not a no-op: neither the run that keeps every pixel with h > 0 nor the run without keep
    y = _gchain(c, c.x0, ts, seed, aux=aux, keep=(c.h, c.k0), thr=THR)
    y_any = _gchain(c, c.x0, ts, seed, aux=aux, keep=((c.h > 0).float(), c.k0), entry="keep")
    y_plain = _gchain(c, c.x0, ts, seed, aux=aux, entry="tile")
    for name, other in (("h > 0", y_any), ("no keep", y_plain)):
        err = max_abs(y.cpu(), other.cpu())
        print(f"{cfg} dim {dim} s={s} halo_x={hx}: gated run vs the {name} run max-abs {err:.3e} (bound {_bound(other):.3e})")
        assert err > _bound(other)


@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_gate_invisible_ends(ctx, cfg, dim, s, B, aux, ts, hx):
    c = ctx(cfg, dim, s, B, hx)
    seed = 535353 + s
    binary = (c.h == 1).float()
    y_keep = _gchain(c, c.x0, ts, seed, aux=aux, keep=(binary, c.k0), entry="keep")
    for thr in (THR, [1e-6, 0.999, 0.37], [1.0, 1.0, 1.0]):
        assert torch.equal(_gchain(c, c.x0, ts, seed, aux=aux, keep=(binary, c.k0), thr=thr), y_keep), thr
    # gt = NULL (and gt->thr = NULL) is sinddm_sample_chain_mix: the soft blend with h as the weight it has always been
    y_mix = _gchain(c, c.x0, ts, seed, aux=aux, keep=(c.h, c.k0), entry="mix")
    assert torch.equal(_gchain(c, c.x0, ts, seed, aux=aux, keep=(c.h, c.k0), gate_null=True), y_mix)
    assert torch.equal(_gchain(c, c.x0, ts, seed, aux=aux, keep=(c.h, c.k0)), y_mix)
    assert torch.equal(_gchain(c, c.x0, ts, seed, aux=aux, keep=(c.h, c.k0), entry="keep"), y_mix)
    assert not torch.equal(_gchain(c, c.x0, ts, seed, aux=aux, keep=(c.h, c.k0), thr=THR), y_mix)


# ---- G4: exact pixels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_gate_exact_pixels(ctx, cfg, dim, s, B, aux, ts, hx):
    c = ctx(cfg, dim, s, B, hx)
    seed = 919191 + s
    assert ts[-1] == 0
    y = c.centre(_gchain(c, c.x0, ts, seed, aux=aux, keep=(c.h, c.k0), thr=THR))
    full = (c.h == 1).expand(B, 3, -1, -1)
    assert torch.equal(y[full], c.k0[None].expand(B, -1, -1, -1)[full])             # h = 1 down to t = 0: the known image
    # the first step alone
    t, thr = ts[0], THR[0]
    k, ab = c.d._coef_table(s)[t], c.d._keep_ab_table()[t]
    y1 = c.centre(_gchain(c, c.x0, [t], seed, aux=aux, keep=(c.h, c.k0), thr=[thr]))
    plain = c.centre(_gchain(c, c.x0, [t], seed, aux=aux, entry="tile"))
    kept, free = (_gated_mask(c.h, thr) == 1).expand(B, 3, -1, -1), (_gated_mask(c.h, thr) == 0).expand(B, 3, -1, -1)
    assert bool(kept.any()) and bool(free.any()) and float(ab[1]) != 0.0
    assert torch.equal(y1[free], plain[free])                                       # h < thr: the plain call's pixel
    z = c.centre(_draw(c, c.x0, seed, 0)).double()
    target = c.k0.double()[None]
    if k.mode == 1:
        target = float(k.gamma_tm1) * c.xt.double() + (1.0 - float(k.gamma_tm1)) * target
    want = float(ab[0]) * target + float(ab[1]) * z
    err, bound = float((y1.double() - want)[kept].abs().max()), _bound(want)
    print(f"{cfg} dim {dim} s={s} halo_x={hx} t={t} mode {k.mode}: kept pixels vs keep_a*target + keep_b*z max-abs {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound
    assert max_abs(y1[kept].cpu(), plain[kept].cpu()) > 1e-2                         # (the kept pixels did move)


# ---- G5: composition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_gate_streams_and_noise_buffer(ctx, cfg, dim, s, B, aux, ts, hx):
    c = ctx(cfg, dim, s, B, hx)
    seed, sid0 = 797 + s, 5
    y0 = _gchain(c, c.x0, ts, seed, sid0=sid0, aux=aux, keep=(c.h, c.k0), thr=THR)
    if aux:
        assert torch.equal(y0, _gchain(c, c.x0, ts, seed, sid0=sid0, aux=False, keep=(c.h, c.k0), thr=THR))
    draws = lambda sd: torch.stack([_draw(c, c.x0, sd, sid0 + i) for i in range(len(ts))]).contiguous()
    assert torch.equal(y0, _gchain(c, c.x0, ts, 0, aux=aux, keep=(c.h, c.k0), thr=THR, noise=draws(seed)))
    assert not torch.equal(y0, _gchain(c, c.x0, ts, 0, aux=aux, keep=(c.h, c.k0), thr=THR, noise=draws(seed + 1)))


@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_gate_per_sample_hold_maps(ctx, cfg, dim, s, B, aux, ts, hx):
    c = ctx(cfg, dim, s, B, hx)
    seed = 383838 + s
    maps = [_hold(c.H, c.W, v) for v in range(4)]
    assert not any(torch.equal(maps[i], maps[j]) for i in range(4) for j in range(i))
    stack = torch.stack([maps[b % 4] for b in range(B)]).contiguous()
    y = _gchain(c, c.x0, ts, seed, aux=aux, keep=(stack, c.k0), thr=THR, per_sample=True)
    for v in range(4):
        y_shared = _gchain(c, c.x0, ts, seed, aux=aux, keep=(maps[v], c.k0), thr=THR)
        rows = list(range(v, B, 4))                                                 # (B = 16: on both sides of the split)
        assert torch.equal(y[rows], y_shared[rows]), f"map {v}"
    assert not torch.equal(y[0], _gchain(c, c.x0, ts, seed, aux=aux, keep=(maps[1], c.k0), thr=THR)[0])


# (setting, the attributes it puts on the diffusion): a gated run of the four levels 3 .. 0 through each unfused tail
UNFUSED = {"jump": dict(resample=(2, 2)), "multistep": dict(solver_order=2),
           "layout": dict(layout_down=3, layout_strength=0.75, layout_t_min=0)}


@pytest.mark.parametrize("setting", list(UNFUSED))
@pytest.mark.parametrize("case", [1, 3], ids=[CASE_IDS[1], CASE_IDS[3]])
def test_gate_through_jump_multistep_and_layout_tails(ctx, case, setting):
    """`_run_steps` twice on the same recorded draws: through the chain call (the jump / multistep / layout kernel with the
    threshold in its TailArgs) and step by step (sinddm_reverse_step_jump / _ms / _layout on the mask (h >= thr) built in
    torch; a step the option does not touch: sinddm_reverse_step_keep_gate)."""
    cfg, dim, s, B, aux, _, hx = CASES[case]
    c = ctx(cfg, dim, s, B, hx)
    d, ts = c.d, [3, 2, 1, 0]
    saved = {k: getattr(d, k) for k in ("resample", "solver_order", "layout_maps", "layout_down", "layout_strength", "layout_t_min")}
    calls = []

    def draws(kind, shape, ss, tt, dev):                                            # (both routes ask in the same order)
        calls.append((kind, tt))
        n = int(np.prod(shape))
        return _fill(n, 5150 + len(calls), 0).view(shape)

    try:
        for k, v in UNFUSED[setting].items():
            setattr(d, k, {s: v} if k == "layout_down" else v)
        if setting == "layout":
            d.layout_maps = {s: (hash_randn((3, c.H, c.W), 77) * 0.5).clamp(-1, 1).to(DEV)}
        d.keep_maps, d.keep_gated, d.noise_fn, d.two_streams = {s: (c.h, c.k0)}, True, draws, aux
        d.chain_noise = False
        ref = d._run_steps(c.x0.clone(), s, ts)
        order, calls[:] = list(calls), []
        d.chain_noise = True
        got = d._run_steps(c.x0.clone(), s, ts)
        assert calls == order and len(order) >= len(ts)
        if setting == "jump":
            assert any(kind == "jump" for kind, _ in order)
        assert torch.isfinite(got).all()
        err, bound = max_abs(got.cpu(), ref.cpu()), _bound(ref)
        print(f"{CASE_IDS[case]} {setting}: gated chain vs stepwise over {len(order)} draws max-abs {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        # the gate acts in that tail: the ungated soft-blend run of the same draws lands elsewhere
        d.keep_gated = False
        calls[:] = []
        assert max_abs(d._run_steps(c.x0.clone(), s, ts).cpu(), got.cpu()) > 1e-3
    finally:
        for k, v in saved.items():
            setattr(d, k, v)
        d.keep_maps, d.keep_gated, d.noise_fn, d.chain_noise = None, False, None, False


# ---- G6: the stepwise kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,t", [(0, 700), (1, 400), (1, 0)], ids=["mode0", "mode1", "mode2"])
def test_reverse_step_keep_gate_against_torch(s, t):
    from sinddm_amd import _lib
    from sinddm_amd.configs import build_diffusion
    lib = _lib.load()
    net, d = build_diffusion("C2", dim=20, device=DEV)
    B, H, W = 3, 48, 53                                                         # odd width, several blocks
    x, eps, xt, z = ((hash_randn((B, 3, H, W), 50 + i) * a).to(DEV) for i, a in enumerate((0.8, 1.0, 0.5, 1.0)))
    h, k0 = _hold(H, W), _known(H, W, 71)
    ew = (0.2 + 0.8 * hash_randn((H, W), 60).abs().clamp(0, 1)).to(DEV)
    ec = (hash_randn((3, H, W), 61) * 0.3).to(DEV)
    k = d.step_coefs(t, s)
    assert k.mode == {(0, 700): 0, (1, 400): 1, (1, 0): 2}[(s, t)]
    st = _lib.stream_ptr(DEV)
    ka, kb = 0.8, 0.6                                                           # (keep_b != 0 at every mode)
    for edit in (False, True):
        e = (_lib.ptr(ew), _lib.ptr(ec)) if edit else (None, None)
        plain = torch.empty_like(x)
        if edit:
            rc = lib.sinddm_reverse_step_edit(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(plain), C.byref(k),
                                              *e, B, 3, H * W, st)
        else:
            rc = lib.sinddm_reverse_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(plain), C.byref(k),
                                         x.numel(), st)
        assert rc == 0
        counts = []
        for thr in (0.4, 0.5, 0.55, 1.0):                                       # below, at and above the 0.5 plateau; at the top one
            out, out_ref = torch.empty_like(x), torch.empty_like(x)
            m = _gated_mask(h, thr)
            rc = lib.sinddm_reverse_step_keep_gate(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(out), C.byref(k),
                                                   *e, _lib.ptr(h), _lib.ptr(k0), ka, kb, B, 3, H * W, st, thr)
            rc2 = lib.sinddm_reverse_step_keep(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(out_ref), C.byref(k),
                                               *e, _lib.ptr(m), _lib.ptr(k0), ka, kb, B, 3, H * W, st)
            torch.cuda.synchronize()
            assert rc == 0 and rc2 == 0
            counts.append(int(m.sum()))
            target = k0[None].expand_as(x)
            if k.mode == 1:
                target = k.gamma_tm1 * xt + (1.0 - k.gamma_tm1) * target
            ref = m * (ka * target + kb * z) + (1 - m) * plain
            err, bound = max_abs(out.cpu(), ref.cpu()), _bound(ref)
            print(f"s={s} t={t} mode {k.mode} edit={edit} thr={thr}: reverse_step_keep_gate vs torch max-abs {err:.3e} "
                  f"(bound {bound:.3e})")
            assert err <= bound
            assert torch.equal(out, out_ref)                                    # the ungated kernel on the gated mask, bit for bit
            sel = (m == 0).expand_as(x)
            assert torch.equal(out[sel], plain[sel])                            # exact where the gate releases
        assert counts[0] == counts[1] > counts[2] > counts[3] > 0              # h == thr counts as kept


# ---- G7: the driver on the C1 pyramid ---------------------------------------------------------------------------------------------------
def test_edit_on_c1(golden, tmp_path):
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    sizes = [tuple(s) for s in meta["image_sizes_hw"]]
    H, W = sizes[-1]
    assert (H, W) == (94, 126) and [w for _, w in sizes] == [64, 90, 126]
    t_list = em.num_timesteps_ideal[1:]
    # a {0, 1} map on a region that is whole footprints at every scale: the columns from 63 on (63 * 90 / 126 = 45, 63 * 64 /
    # 126 = 32; no row other than 0 and 94 divides that way) -- asserted on the CPU first
    strength = torch.zeros(H, W)
    strength[:, 63:] = 1
    holds, masks = hold_pyramid(strength, sizes), keep_mask_pyramid(1 - strength, sizes, hard=True)
    for hd, m, (h, w), x0 in zip(holds, masks, sizes, (32, 45, 63)):
        assert torch.equal(hd, m) and torch.equal(hd, torch.cat([torch.ones(h, x0), torch.zeros(h, w - x0)], 1))
    seeds = [11, 12]
    em.draw_log = []
    outs = tr.edit(strength, batch_size=2, custom_t_list=t_list, seeds=seeds, save_images=False)
    log, em.draw_log = em.draw_log, None
    assert em.keep_maps is None and em.keep_gated is False
    assert [e[0] for e in log] == ["init", "chain_seeds", "renoise", "chain_seeds", "renoise", "chain_seeds"]   # one chain per scale
    assert [tuple(o.shape) for o in outs] == [(2, 3) + hw for hw in sizes] and all(torch.isfinite(o).all() for o in outs)
    ref = tr.inpaint(1 - strength, batch_size=2, hard=True, custom_t_list=t_list, seeds=seeds, save_images=False)
    assert all(torch.equal(a, b) for a, b in zip(outs, ref))                    # a binary map is inpaint, bit for bit
    for s, x0 in enumerate((32, 45, 63)):                                       # strength 0: the scale's known image, exactly
        known = tr.data_list[s][0][0]
        assert torch.equal(outs[s][:, :, :, :x0], known[None].expand(2, -1, -1, -1)[:, :, :, :x0])
    diff = max_abs(outs[-1][0][:, :, 63:].cpu(), outs[-1][1][:, :, 63:].cpu())
    print(f"edit C1 dim 32 T=20 B=2: the two samples differ where strength = 1 by max-abs {diff:.3e}")
    assert diff > 1e-2
    # without seeds the run is one torch-seeded chain per scale, like inpaint's
    em.draw_log = []
    torch.manual_seed(2468)
    tr.edit(strength, batch_size=2, custom_t_list=t_list, save_images=False)
    log, em.draw_log = em.draw_log, None
    assert [e[0] for e in log] == ["init", "chain", "renoise", "chain", "renoise", "chain"]
    # a (B, H, W) stack: sample b is the shared run with b's map; gray levels release in between
    gray = torch.zeros(H, W)
    gray[20:70, 30:100] = 0.5
    gray[40:60, 50:80] = 1
    stack = torch.stack([strength, gray, 1 - strength])
    seeds3 = [21, 22, 23]
    per = tr.edit(stack, batch_size=3, custom_t_list=t_list, seeds=seeds3, save_images=False)
    for b in range(3):
        one = tr.edit(stack[b], batch_size=3, custom_t_list=t_list, seeds=seeds3, save_images=False)
        assert all(torch.equal(p[b], o[b]) for p, o in zip(per, one)), f"sample {b}"
    known = tr.data_list[-1][0][0]
    untouched = (gray == 0).to(DEV)
    assert torch.equal(per[-1][1][:, untouched], known[:, untouched])           # strength 0 of the gray map: kept exactly
    half = (gray == 0.5).to(DEV)
    assert max_abs(per[-1][1][:, half].cpu(), known[:, half].cpu()) > 1e-3      # strength 0.5: released on the way, it moved
    # an image of its own, and the errors; both put the options back
    pic = (hash_randn((3, H, W), 5) * 0.5).clamp(-1, 1)
    own = tr.edit(gray, image=pic, batch_size=2, custom_t_list=t_list, seeds=seeds, save_images=False)
    assert torch.equal(own[-1][0][:, untouched], pic.to(DEV)[:, untouched])
    for bad in (dict(strength=gray[:-1]), dict(strength=gray * 2), dict(strength=gray, image=pic[:, :-1]),
                dict(strength=gray, image=pic * 3), dict(strength=gray, scale_mul=(1, 2)), dict(strength=stack[:2], batch_size=3)):
        with pytest.raises(ValueError):
            tr.edit(**{"batch_size": 2, "save_images": False, **bad})
        assert em.keep_maps is None and em.keep_gated is False
