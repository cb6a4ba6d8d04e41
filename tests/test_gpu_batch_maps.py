"""Per-sample conditioning maps inside the fused sampler chain (sinddm_sample_chain_batch; a leading batch dimension on
`keep_maps` / `layout_maps`, `layout_gain`, `roi_bbs_batch`): every sample of a batch is its own edit job.

The yardstick is the project's own shared-map entry (sinddm_sample_chain_layout and the entries below it), which this feature
must not change: a per-sample run is compared with shared runs that get one sample's maps.
  1. equal rows are the shared run, bit for bit: edit, keep, keep + edit, layout, keep + jump on every tail kernel's shape;
  2. a sample sees only its own maps: sample b of the per-sample run is sample b of the shared run with b's maps (after the
     pre-check that, with shared maps, a sample does not depend on the other samples' start states); in-kernel Philox,
     per-sample seeds, recorded noise;
  3. exact ends: mask rows of all 0 / all 1;
  4. `layout_gain`: the fp32 product g_i * gain_b, N = 1 replaces x_recon by L[b], gain 0 is the plain sample;
  5. the public route: `_run_steps` is the direct call and agrees with the `_p_sample_host_t` loop;
  6. every SINDDM_E_BADARG of the new entry, none of which touches the device; wrong leading dimensions from Python;
  7. `inpaint` / `outpaint` / `paint2image` with two jobs on the C1 pyramid.
Shapes: the four of test_gpu_chain_guided.SHAPES (one tail kernel each; three steps incl. t = 0) and the tiled case of
test_gpu_keep.CASES.  Probe samples: both sides of the two-stream split.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import max_abs
from sinddm_amd.synth import hash_randn
from test_gpu_chain_guided import _trainer
from test_gpu_keep import CASE_IDS, CASES, _bound, _Ctx, _draw
from test_gpu_resample import _jump_array, _walk
from test_gpu_seeds import _dev_seeds, _seed_list

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_LAY = 11                    # 48, 64, 67, 90, 133, 177 all leave a partial block: edge blocks on both axes of every shape
G_LAY = (1.0, 0.5, 0.0)       # the strengths of the three steps: the last one keeps its fused tail
BADARG = -1


def _probes(B):
    Bh0 = (B + 1) // 2
    return sorted({0, Bh0 - 1, Bh0, B - 1})


def _maps(c, B, key=500):
    """Random per-sample maps at the centre size, every row different: ew (B,H,W), ec (B,3,H,W), mask (B,H,W) with hard and
    soft pixels, known image (B,3,H,W), layout (B,3,H,W)."""
    H, W = c.H, c.W
    r = hash_randn((B, H, W), key + 2)
    m = torch.where(r > 0.4, torch.ones_like(r), torch.where(r < -0.4, torch.zeros_like(r), torch.full_like(r, 0.25)))
    out = dict(ew=0.2 + 0.8 * hash_randn((B, H, W), key).abs().clamp(0, 1), ec=hash_randn((B, 3, H, W), key + 1) * 0.3, m=m,
               k0=(hash_randn((B, 3, H, W), key + 3) * 0.6).clamp(-1, 1), lay=(hash_randn((B, 3, H, W), key + 4) * 0.6).clamp(-1, 1))
    out = {k: v.to(DEV).contiguous() for k, v in out.items()}
    for v in out.values():
        assert not torch.equal(v[0], v[1]) and not torch.equal(v[0], v[-1])
    return out


def _run(c, x0, ts, seed=0, sid0=0, aux=False, edit=None, keep=None, lay=None, g=G_LAY, N=N_LAY, gain=None, jump_to=None,
         noise=None, jnoise=None, seeds=None, entry="batch", flags=None, gain_ptr=None, ptr_shift=None, expect_rc=0):
    """One chain call on centre-size arguments of a test_gpu_keep._Ctx, extended here; the extended result.  A map with a
    leading batch dimension is per sample.  entry = 'batch': sinddm_sample_chain_batch with the flags read off the maps'
    dimensions (or `flags`, four ints); 'layout': sinddm_sample_chain_layout, shared maps only.  `ptr_shift`: {name: bytes}
    added to a map's pointer (misalignment cases); `gain_ptr`: a raw pointer in place of `gain`."""
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
    shift = ptr_shift or {}
    p = lambda name, t: None if t is None else _lib.ptr(t) + shift.get(name, 0)
    held = {}                                                # (extended maps: alive until the synchronise below)
    opts = _lib.ChainOpts()
    if edit is not None:
        held["ew"], held["ec"] = c.ext(edit[0]), c.ext(edit[1])
        opts.edit_w, opts.edit_c = p("ew", held["ew"]), p("ec", held["ec"])
    opts.noise = _lib.ptr(noise)
    kopts = None
    if keep is not None:
        held["m"], held["k0"] = c.ext(keep[0]), c.ext(keep[1])
        ab_tab = c.d._keep_ab_table()
        ab = (C.c_float * (2 * n))(*[float(v) for t in ts for v in ab_tab[t]])
        kopts = _lib.KeepOpts()
        kopts.mask, kopts.x0, kopts.ab = p("m", held["m"]), p("k0", held["k0"]), C.cast(ab, C.POINTER(C.c_float))
    sd = _dev_seeds(seeds) if seeds is not None else None
    ropts = None
    if jump_to is not None:
        jumps = _jump_array(c, ts, jump_to)
        ropts = _lib.ResampleOpts()
        ropts.jumps, ropts.noise = C.cast(jumps, C.POINTER(_lib.JumpCoefs)), _lib.ptr(jnoise)
    lopts = None
    if lay is not None:
        held["lay"] = c.ext(lay)
        h, w = -(-H // N), -(-(We - 2 * c.hx) // N)
        held["delta"] = torch.full((B, 3, h, w), 7.5, device=DEV)
        garr = (C.c_float * n)(*[float(v) for v in g[:n]])
        lopts = _lib.LayoutOpts()
        lopts.layout, lopts.down, lopts.g, lopts.delta = p("lay", held["lay"]), N, C.cast(garr, C.POINTER(C.c_float)), \
            _lib.ptr(held["delta"])
    ref = lambda o: C.byref(o) if o is not None else None
    args = [_lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
            coefs, tl, n, float(c.s), seed, sid0, c.dim, B, H, We - 2 * c.hx, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
            _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, c.hx, ref(kopts), _lib.ptr(sd), ref(ropts), ref(lopts)]
    per = (int(edit is not None and edit[0].dim() == 3), int(keep is not None and keep[0].dim() == 3),
           int(keep is not None and keep[1].dim() == 4), int(lay is not None and lay.dim() == 4))
    if entry == "layout":
        assert not any(per) and gain is None and flags is None
        rc = lib.sinddm_sample_chain_layout(*args)
    else:
        held["gain"] = gain
        bo = _lib.BatchOpts(*(flags if flags is not None else per), gain_ptr if gain_ptr is not None else _lib.ptr(gain))
        rc = lib.sinddm_sample_chain_batch(*args, C.byref(bo))
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    if rc != 0:
        assert torch.equal(xa, c.ext(x0))                    # refused before any device work
        return None
    assert flag.value in (0, 1)
    return xb if flag.value == 1 else xa


# the conditioning of one kind of run: which of the per-sample maps it takes, whether it jumps
KINDS = {"edit": ("edit",), "keep": ("keep",), "keep_edit": ("keep", "edit"), "layout": ("lay",), "keep_jump": ("keep", "jump"),
         "all": ("keep", "edit", "lay")}


def _kw(kind, mp, ts, s, rows=None):
    """Keyword arguments of `_run` for a kind: `rows` = None takes the per-sample maps, an int the shared maps of that row;
    also the step list (the jump kinds walk test_gpu_resample's five-evaluation walk)."""
    sel = (lambda v: v) if rows is None else (lambda v: v[rows].clone())     # (its own allocation: 16-byte aligned)
    kw, use = {}, KINDS[kind]
    if "edit" in use:
        kw["edit"] = (sel(mp["ew"]), sel(mp["ec"]))
    if "keep" in use:
        kw["keep"] = (sel(mp["m"]), sel(mp["k0"]))
    if "lay" in use:
        kw["lay"] = sel(mp["lay"])
    if "jump" in use:
        ts, kw["jump_to"] = _walk(s)
    return ts, kw


# ---- 1: equal rows are the shared run ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_equal_rows_are_the_shared_run(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    mp = _maps(c, B)
    same = {k: v[3:4].expand_as(v).contiguous() for k, v in mp.items()}          # B copies of row 3
    for kind in ("edit", "keep", "keep_edit", "layout", "keep_jump"):
        seed = 313131 + s
        tk, per = _kw(kind, same, ts, s)
        _, shared = _kw(kind, mp, ts, s, rows=3)
        y = _run(c, c.x0, tk, seed, aux=aux, **per)
        y_ref = _run(c, c.x0, tk, seed, aux=aux, entry="layout", **shared)
        assert torch.isfinite(y).all()
        assert torch.equal(y, y_ref), (kind, max_abs(y.cpu(), y_ref.cpu()))
        # bo with every member zero is the shared entry too
        assert torch.equal(_run(c, c.x0, tk, seed, aux=aux, **shared), y_ref), kind
        # ... and the maps are at work: the unconditioned run lands elsewhere
        plain = _run(c, c.x0, tk, seed, aux=aux, entry="layout", **({"jump_to": shared["jump_to"]} if "jump_to" in shared else {}))
        assert max_abs(plain.cpu(), y.cpu()) > 1e-3, kind


# ---- 2: a sample sees only its own maps ------------------------------------------------------------------------------------------
def _own_maps(c, mp, ts, s, aux, kinds, label, **noise_kw):
    """For every kind: the pre-check (shared maps: sample b does not depend on the other samples' start states), then
    sample b of the per-sample run against sample b of the shared run with b's maps -- torch.equal where the pre-check
    held, test_gpu_keep._bound where it did not."""
    B = c.x0.shape[0]
    other = (hash_randn(tuple(c.x0.shape), 977) * 0.8).to(DEV)
    for kind in kinds:
        tk, per = _kw(kind, mp, ts, s)
        nk = dict(noise_kw)
        if "noise" in nk:                                    # recorded draws: the stream's own numbers, as a buffer
            nk["noise"] = torch.stack([_draw(c, c.x0, nk["seed"], i) for i in range(len(tk))]).contiguous()
            nk["seed"] = 0
        y = _run(c, c.x0, tk, aux=aux, **per, **nk)
        assert torch.isfinite(y).all()
        for b in _probes(B):
            _, shared = _kw(kind, mp, ts, s, rows=b)
            y_b = _run(c, c.x0, tk, aux=aux, entry="layout", **shared, **nk)
            x_alt = other.clone()
            x_alt[b] = c.x0[b]
            indep = torch.equal(_run(c, x_alt, tk, aux=aux, entry="layout", **shared, **nk)[b], y_b[b])
            err, bound = max_abs(y[b].cpu(), y_b[b].cpu()), _bound(y_b[b])
            print(f"{label} {kind} sample {b} of {B}: pre-check (shared maps, other samples' starts changed) "
                  f"{'bit-equal' if indep else 'NOT bit-equal'}; per-sample vs shared-with-own-maps max-abs {err:.3e}")
            if indep:
                assert torch.equal(y[b], y_b[b]), (kind, b, err)
            else:
                assert err <= bound, (kind, b, err, bound)
        # every row is conditioned on something else: the samples next to a probe do not equal the probe's shared run
        assert not torch.equal(y[1], _run(c, c.x0, tk, aux=aux, entry="layout", **_kw(kind, mp, ts, s, rows=0)[1], **nk)[1])


@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_a_sample_sees_only_its_own_maps_philox(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    _own_maps(c, _maps(c, B), ts, s, aux, ("edit", "keep_edit", "all", "keep_jump"), f"{cfg} dim {dim} s={s} halo_x={hx} philox",
              seed=717171 + s, sid0=3)


@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_a_sample_sees_only_its_own_maps_seeded(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    _own_maps(c, _maps(c, B, 600), ts, s, aux, ("all", "keep_jump"), f"{cfg} dim {dim} s={s} halo_x={hx} seeds",
              seeds=_seed_list(B), sid0=(s << 32) | 2)


@pytest.mark.parametrize("idx", [1, 3], ids=[CASE_IDS[1], CASE_IDS[3]])
def test_a_sample_sees_only_its_own_maps_recorded_noise(idx):
    cfg, dim, s, B, aux, ts, hx = CASES[idx]
    c = _Ctx(cfg, dim, s, B, hx)
    _own_maps(c, _maps(c, B, 700), ts, s, aux, ("keep_edit", "all"), f"{cfg} dim {dim} s={s} recorded noise", seed=5151 + s,
              noise=True)


# ---- 3: exact ends -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_exact_ends_per_sample(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    mp = _maps(c, B)
    seed = 424242 + s
    assert ts[-1] == 0
    m = torch.zeros(B, c.H, c.W, device=DEV)
    m[1::2] = 1.0                                            # rows alternate all-0 and all-1
    y = c.centre(_run(c, c.x0, ts, seed, aux=aux, keep=(m, mp["k0"])))
    plain = c.centre(_run(c, c.x0, ts, seed, aux=aux, entry="layout"))
    assert torch.equal(y[0::2], plain[0::2])                 # m == 0: the plain chain's samples, bit for bit
    assert torch.equal(y[1::2], mp["k0"][1::2])              # m == 1 down to t = 0: each sample's own known image
    assert not torch.equal(y[1], plain[1])
    # the mask alone per sample, the known image shared
    y = c.centre(_run(c, c.x0, ts, seed, aux=aux, keep=(m, mp["k0"][2].clone())))
    assert torch.equal(y[0::2], plain[0::2]) and torch.equal(y[1::2], mp["k0"][2][None].expand_as(y[1::2]))


# ---- 4: layout_gain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_layout_gain(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    mp = _maps(c, B)
    seed = 858585 + s
    L = mp["lay"][0].clone()
    gain_h = (0.05 + 0.9 * hash_randn((B,), 41).abs().clamp(0, 1)).numpy().astype(np.float32)
    gain_h[_probes(B)[1]] = 0.0                              # one probe's gain is 0, one 1
    gain_h[_probes(B)[-1]] = 1.0
    gain = torch.from_numpy(gain_h).to(DEV)
    g = (0.75, 0.5, 0.0)
    y = _run(c, c.x0, ts, seed, aux=aux, lay=L, g=g, gain=gain)
    plain = _run(c, c.x0, ts, seed, aux=aux, entry="layout")
    for b in _probes(B):
        gb = [float(np.float32(v) * gain_h[b]) for v in g]   # the fp32 product, formed once
        y_b = _run(c, c.x0, ts, seed, aux=aux, entry="layout", lay=L, g=gb)
        assert torch.equal(y[b], y_b[b]), (b, max_abs(y[b].cpu(), y_b[b].cpu()))
        if gain_h[b] == 0.0:                                 # no pull: the plain sample, though the steps ran unfused
            err, bound = max_abs(y[b].cpu(), plain[b].cpu()), _bound(plain[b])
            print(f"{cfg} dim {dim} s={s} halo_x={hx}: gain 0 vs the plain run's sample max-abs {err:.3e} (bound {bound:.3e})")
            assert err <= bound
        else:
            assert max_abs(y[b].cpu(), plain[b].cpu()) > 1e-4
    # gain 1 is no gain; and N = 1, g = 1, gain = 1 at t = 0 replaces x_recon by L[b]: the step returns clamp(L[b]) = L[b]
    ones = torch.ones(B, device=DEV)
    y1 = _run(c, c.x0, [0], seed, aux=aux, lay=mp["lay"], g=(1.0,), N=1, gain=ones)
    assert torch.equal(y1, _run(c, c.x0, [0], seed, aux=aux, lay=mp["lay"], g=(1.0,), N=1))
    err, bound = max_abs(c.centre(y1).cpu(), mp["lay"].cpu()), _bound(mp["lay"])
    print(f"{cfg} dim {dim} s={s} halo_x={hx}: N = 1, g = 1, gain = 1 at t = 0 vs L[b] max-abs {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ---- 5: the public route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_run_steps_with_per_sample_maps(cfg, dim, s, B, aux, ts, hx):
    c = _Ctx(cfg, dim, s, B, hx)
    d, mp, seed = c.d, _maps(c, B), 616161 + s
    # two box lists in turn (the scale's boxes, and the first of them alone) -> per-sample edit maps
    d.roi_guided_sampling = True
    d.roi_bbs_batch = [d.roi_bbs if b % 2 == 0 else d.roi_bbs[:1] for b in range(B)]
    ew, ec = d.roi_edit_maps(s, c.H, c.W, DEV)
    assert tuple(ew.shape) == (B, c.H, c.W) and tuple(ec.shape) == (B, 3, c.H, c.W)
    assert torch.equal(ew[0], c.ew) and torch.equal(ec[0], c.ec) and not torch.equal(ew[1], c.ew)       # row b: built as the shared pair is
    gain_h = (0.05 + 0.9 * hash_randn((B,), 43).abs().clamp(0, 1)).numpy().astype(np.float32)
    d.keep_maps = {s: (mp["m"], mp["k0"])}
    d.layout_maps, d.layout_down, d.layout_strength, d.layout_t_min = {s: mp["lay"]}, {s: N_LAY}, 0.75, ts[1]
    d.layout_gain = gain_h.tolist()
    g = (0.75, 0.75, 0.0)
    direct = dict(edit=(ew, ec), keep=(mp["m"], mp["k0"]), lay=mp["lay"], g=g, gain=torch.from_numpy(gain_h).to(DEV))
    x = c.x0.clone()
    for i, t in enumerate(ts):
        z = c.centre(_draw(c, c.x0, seed, i))
        d.noise_fn = lambda kind, shape, ss, tt, dev, z=z: z
        x = d._p_sample_host_t(x, t, s)
    d.noise_fn = None
    y = _run(c, c.x0, ts, seed, aux=aux, **direct)
    err, bound = max_abs(c.centre(y).cpu(), x.cpu()), _bound(x)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B}: per-sample chain vs B = 1 step calls max-abs {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound
    outs = {}
    for two in (aux, not aux):
        torch.manual_seed(11)
        seed_api = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
        torch.manual_seed(11)
        d.two_streams = two
        d.draw_log = []
        outs[two] = d._run_steps(c.x0.clone(), s, ts)
        log, d.draw_log = d.draw_log, None
        assert len(log) == 1 and log[0][0] == ("chain_tile" if hx else "chain") and log[0][2] == seed_api   # entries unchanged
    assert torch.equal(outs[True], outs[False])
    assert torch.equal(outs[aux], c.centre(_run(c, c.x0, ts, seed_api, aux=aux, **direct)))


# ---- 6: error returns ----------------------------------------------------------------------------------------------------------
def test_batch_entry_refuses_misuse_before_any_device_work():
    cfg, dim, s, B, aux, ts, hx = CASES[0]                   # 48x64: the plain fused route
    c = _Ctx(cfg, dim, s, B, hx)
    mp = _maps(c, B)
    L, gain = mp["lay"], torch.ones(B, device=DEV)
    bad = lambda **kw: _run(c, c.x0, ts, 1, expect_rc=BADARG, **kw)
    # a flag set whose pointer is NULL
    bad(flags=(1, 0, 0, 0))
    bad(flags=(0, 1, 0, 0))
    bad(flags=(0, 0, 1, 0))
    bad(flags=(0, 0, 0, 1))
    bad(flags=(0, 0, 0, 1), keep=(mp["m"], mp["k0"]), edit=(mp["ew"], mp["ec"]))         # (the others set, the layout not)
    # layout_gain without a layout; not 4-byte aligned
    bad(gain=gain)
    bad(gain=gain, keep=(mp["m"], mp["k0"]))
    bad(lay=L, gain_ptr=gain.data_ptr() + 2)
    # per-sample slices off the 16-byte rule of the plain fused route
    room = lambda t: torch.cat([t.reshape(-1), t.new_zeros(4)]).view(-1)[:t.numel()].view_as(t)       # (4 floats behind the map)
    bad(keep=(room(mp["m"]), mp["k0"]), ptr_shift={"m": 4})
    bad(keep=(mp["m"], room(mp["k0"])), ptr_shift={"k0": 8})
    bad(edit=(room(mp["ew"]), mp["ec"]), ptr_shift={"ew": 4})
    assert _run(c, c.x0, ts, 1, lay=L, gain=gain) is not None                              # (the good call goes through)


def test_python_refuses_a_wrong_leading_dimension():
    from sinddm_amd import _lib
    cfg, dim, s, B, aux, ts, hx = CASES[0]
    c = _Ctx(cfg, dim, s, B, hx)
    d, mp = c.d, _maps(c, B)
    d.keep_maps = {s: (mp["m"][:B - 1].contiguous(), mp["k0"])}
    with pytest.raises(_lib.SinddmError, match="keep_maps"):
        d._run_steps(c.x0.clone(), s, ts)
    d.keep_maps = {s: (mp["m"], mp["k0"][:3].contiguous())}
    with pytest.raises(_lib.SinddmError, match="keep_maps"):
        d._p_sample_host_t(c.x0.clone(), ts[0], s)
    d.keep_maps = None
    d.layout_maps, d.layout_down = {s: mp["lay"][:2].contiguous()}, {s: N_LAY}
    with pytest.raises(_lib.SinddmError, match="layout_maps"):
        d._run_steps(c.x0.clone(), s, ts)
    d.layout_maps = {s: mp["lay"]}
    for bad in ([0.5] * (B - 1), [0.5] * (B - 1) + [1.5]):
        d.layout_gain = bad
        with pytest.raises(ValueError, match="layout_gain"):
            d._run_steps(c.x0.clone(), s, ts)
    d.layout_gain, d.layout_maps = None, None
    d.roi_guided_sampling, d.roi_bbs_batch = True, [d.roi_bbs] * (B - 1)
    with pytest.raises(ValueError, match="roi_bbs_batch"):
        d._p_sample_host_t(c.x0.clone(), ts[0], s)
    with pytest.raises(ValueError, match="roi_bbs_batch"):
        d._run_steps(c.x0.clone(), s, ts)


# ---- 7: end to end on the C1 pyramid ---------------------------------------------------------------------------------------------
def test_two_jobs_per_call_on_c1(golden, tmp_path):
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    sizes = [tuple(sz) for sz in meta["image_sizes_hw"]]
    H, W = sizes[-1]
    img = tr.data_list[-1][0][0]
    kw = dict(batch_size=2, custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    masks = torch.ones(2, H, W)
    masks[0, 31:61, 43:83] = 0                               # two different holes
    masks[1, 10:40, 90:130] = 0
    em.draw_log = []
    torch.manual_seed(2468)
    outs = tr.inpaint(masks, **kw)
    log, em.draw_log = em.draw_log, None
    assert em.keep_maps is None
    assert [e[0] for e in log] == ["init", "chain", "renoise", "chain", "renoise", "chain"]      # still one chain per scale
    assert [tuple(o.shape) for o in outs] == [(2, 3) + hw for hw in sizes] and all(torch.isfinite(o).all() for o in outs)
    kept = masks.bool().to(DEV)
    for b in (0, 1):
        assert torch.equal(outs[-1][b][:, kept[b]], img[:, kept[b]])                             # its own mask: exact
        hole = ~kept[b]                                                                          # (kept under the other's mask)
        assert bool(kept[1 - b][hole].all()) and max_abs(outs[-1][b][:, hole].cpu(), img[:, hole].cpu()) > 1e-2
    with pytest.raises(ValueError):
        tr.inpaint(torch.ones(3, H, W), **kw)
    # outpaint: two anchors, the training image sits exactly at each sample's own offset
    outs = tr.outpaint((1, 1.5), anchor=[(0.5, 0.0), (0.5, 1.0)], **kw)
    assert em.keep_maps is None
    Wc = int(W * 1.5)
    assert tuple(outs[-1].shape) == (2, 3, H, Wc) and torch.isfinite(outs[-1]).all()
    assert torch.equal(outs[-1][0][:, :, :W], img) and torch.equal(outs[-1][1][:, :, Wc - W:], img)
    assert not torch.equal(outs[-1][1][:, :, :W], img)
    with pytest.raises(ValueError):
        tr.outpaint((1, 1.5), anchor=[(0.5, 0.0)] * 3, **kw)
    # paint2image: two layouts, two strengths
    lay = torch.stack([img.cpu().flip(-1), -img.cpu()])
    outs = tr.paint2image(lay, strength=[1.0, 0.5], down=8, **kw)
    assert em.layout_maps is None and em.layout_gain is None
    assert torch.isfinite(outs[-1]).all() and max_abs(outs[-1][0].cpu(), outs[-1][1].cpu()) > 1e-2
