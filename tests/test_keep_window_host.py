"""CPU: windowed known-region sampling (MultiScaleGaussianDiffusion.keep_window).
  1. functions.keep_windows: the geometry of the windows;
  2. the statement in float64, with the oracle's network: a keep run on the window "bounding box of the free pixels, grown by
     16" equals the full run on the free pixels, is the full run's known pixels exactly, and a window grown by 0 is not it;
  3. sampler.RunPlan: the `window` field, the 'window' noise kind, every refusal before any library call, the `draw_log` entry;
     main.py's --keep_window; the entry's argument errors (no launch: safe without a GPU)."""
import pytest
import torch

from oracle import sinddm_oracle as O
from sinddm_amd import _lib
from sinddm_amd.configs import build_diffusion
from sinddm_amd.functions import keep_windows
from sinddm_amd.sampler import NOT_BUILT, RunPlan
from sinddm_amd.synth import hash_randn, he_state_dict
from tile_train_util import sched_in


def _grown(free, g):
    """Per sample (y0, y1, x0, x1) of the bounding box of `free` grown by g and clipped, from the sentence, or None."""
    H, W = free.shape[-2:]
    out = []
    for fb in free.reshape(-1, H, W):
        pts = [(y, x) for y in range(H) for x in range(W) if bool(fb[y, x])]
        if not pts:
            out.append(None)
            continue
        ys, xs = [p[0] for p in pts], [p[1] for p in pts]
        out.append((max(min(ys) - g, 0), min(max(ys) + 1 + g, H), max(min(xs) - g, 0), min(max(xs) + 1 + g, W)))
    return out


def _check(free, g, got):
    """The properties of the issue's sentence for a result that is not None."""
    H, W = free.shape[-2:]
    h, w, org = got
    boxes = _grown(free, g)
    assert org.dtype == torch.int32 and org.device.type == "cpu" and tuple(org.shape) == (len(boxes), 2)
    live = [b for b in boxes if b is not None]
    assert h == max(b[1] - b[0] for b in live)
    w_raw = max(b[3] - b[2] for b in live)
    assert w == (-(-w_raw // 4) * 4 if -(-w_raw // 4) * 4 <= W else w_raw)
    assert (h, w) != (H, W) and h <= H and w <= W
    for b, (oy, ox) in zip(boxes, org.tolist()):
        assert 0 <= oy <= H - h and 0 <= ox <= W - w                       # origins in range
        if b is None:
            assert (oy, ox) == (0, 0)
        else:
            assert oy <= b[0] and b[1] <= oy + h and ox <= b[2] and b[3] <= ox + w      # the grown box inside its window


# ---- 1: geometry ---------------------------------------------------------------------------------------------------------
def test_keep_windows_geometry():
    H, W = 50, 61
    f = torch.zeros(H, W, dtype=torch.bool)
    f[:7, W - 9:] = True                                                   # touches the top and the right border
    got = keep_windows(f, 16)
    _check(f, 16, got)
    assert (got[0], got[1]) == (23, 28) and got[2].tolist() == [[0, W - 28]]          # (25 columns, rounded up to 28)
    assert keep_windows(f, 16, batch=3)[2].tolist() == [[0, W - 28]] * 3              # a shared map: one origin, replicated
    # the grown box exceeds the image on one axis only: the window spans that axis, not the other
    f = torch.zeros(H, W, dtype=torch.bool)
    f[10:40, 20:30] = True
    got = keep_windows(f, 16)
    _check(f, 16, got)
    assert got[0] == H and got[1] == 44 and got[2].tolist() == [[0, 4]]
    # no free pixel; a window that spans the scale
    assert keep_windows(torch.zeros(H, W, dtype=torch.bool), 16) is None
    assert keep_windows(torch.zeros(2, H, W, dtype=torch.bool), 0) is None
    assert keep_windows(torch.ones(H, W, dtype=torch.bool), 0) is None
    f = torch.zeros(H, W, dtype=torch.bool)
    f[20, 20] = f[30, 41] = True
    assert keep_windows(f, 20) is None and keep_windows(f, 16) is not None
    # three per-sample holes of different sizes, one sample without a hole
    f = torch.zeros(4, H, W, dtype=torch.bool)
    f[0, 5:9, 6:12] = True
    f[1, 30:47, 50:61] = True
    f[3, 22, 3] = True
    for g in (0, 3, 16):
        got = keep_windows(f, g)
        _check(f, g, got)
        assert got[2][2].tolist() == [0, 0]
    # w % 4 == 0 whenever w < W allows it; a width whose round-up passes W stays as it is
    f = torch.zeros(H, W, dtype=torch.bool)
    f[25, 20:25] = True                                                    # 5 + 32 = 37 -> 40
    assert keep_windows(f, 16)[1] == 40
    f[25, 4:30] = True                                                     # 0 .. 46 -> 46 -> 48
    assert keep_windows(f, 16)[1] == 48
    f[25, 4:43] = True                                                     # 0 .. 59 -> 59; 60 <= 61 -> 60
    assert keep_windows(f, 16)[1] == 60
    f = torch.zeros(H, 62, dtype=torch.bool)
    f[25, 4:45] = True                                                     # 0 .. 61 -> 61; 64 > 62 -> stays 61
    assert keep_windows(f, 16)[1] == 61
    # a float mask compared by the caller, an int map, numpy-free: any bool-like map
    assert keep_windows((torch.rand(H, W) < 2).to(torch.uint8), 0) is None
    for bad in (-1, 1.5, "16", None, True):
        with pytest.raises(_lib.SinddmError, match="margin"):
            keep_windows(f, bad)


# ---- 2: the statement in float64 -----------------------------------------------------------------------------------------
H2, W2, S2, STEPS2 = 40, 44, 1, [2, 1, 0]                                  # (modes 1, 1, 2 at scale 1)


def _keep_run(sched, sd, x, xt, m, k0, zs, omega):
    """The keep run in float64, from step_tail.h's sentence: out = m * (ka * target + kb * z) + (1 - m) * step."""
    g_row = sched["gammas"][S2 - 1].reshape(-1).clamp(0, 0.55)
    torch.set_default_dtype(torch.float64)                                 # (the oracle builds its embeddings in the default dtype)
    try:
        for t, z in zip(STEPS2, zs):
            y = O.p_sample(sched, sd, x, t, S2, z, xt, omega=omega)
            if t > 0:
                ka, kb = sched["sqrt_alphas_cumprod"][t - 1], sched["sqrt_one_minus_alphas_cumprod"][t - 1]
                target = g_row[t - 1] * xt + (1 - g_row[t - 1]) * k0
            else:
                ka, kb, target = 1.0, 0.0, k0
            x = m * (ka * target + kb * z) + (1 - m) * y
    finally:
        torch.set_default_dtype(torch.float32)
    return x


@pytest.fixture(scope="module")
def statement(golden):
    meta = golden("g11_img_scales.json")["C1"]
    sched = sched_in(O.make_schedule(meta["T"], meta["n_scales"], meta["rescale_losses"], 1, train_full_t=True), torch.float64)
    sd = {k: v.to(torch.float64) for k, v in he_state_dict(16).items()}
    f64 = lambda shape, key, a=1.0: hash_randn(shape, key).to(torch.float64) * a
    x, xt, k0 = f64((1, 3, H2, W2), 31, 0.8), f64((1, 3, H2, W2), 32, 0.5), f64((1, 3, H2, W2), 33, 0.6).clamp(-1, 1)
    zs = [f64((1, 3, H2, W2), 40 + i) for i in range(len(STEPS2))]
    m = torch.ones(H2, W2, dtype=torch.float64)
    m[17:23, 18:25] = 0                                                    # a 6x7 hole ...
    m[19, 25] = 0.5                                                        # ... and one soft pixel
    full = _keep_run(sched, sd, x, xt, m, k0, zs, 0.3)
    return dict(sched=sched, sd=sd, x=x, xt=xt, k0=k0, zs=zs, m=m, full=full)


def _windowed(c, margin):
    h, w, org = keep_windows(c["m"] < 1, margin)
    (oy, ox), = org.tolist()
    win = lambda t: t[..., oy:oy + h, ox:ox + w]
    y = _keep_run(c["sched"], c["sd"], win(c["x"]), win(c["xt"]), win(c["m"]), win(c["k0"]), [win(z) for z in c["zs"]], 0.3)
    out = c["k0"].clone()                                                  # (the run lands clean: the kept value is the known image)
    out[..., oy:oy + h, ox:ox + w] = y
    return out, (h, w, oy, ox)


def test_window_of_margin_16_is_the_full_run_in_float64(statement):
    c = statement
    free = (c["m"] < 1).expand(1, 3, -1, -1)
    assert int(free[0, 0].sum()) == 43 and bool(((c["m"] > 0) & (c["m"] < 1)).any())
    out, (h, w, oy, ox) = _windowed(c, 16)
    assert (h, w) == (38, 40) and (h, w) != (H2, W2) and (oy, ox) == (1, 2)
    err = float((out - c["full"])[free].abs().max())
    print(f"float64 windowed (margin 16, {h}x{w} at ({oy},{ox})) vs full keep run, free pixels: max-abs {err:.3e}")
    assert err <= 1e-12
    assert torch.equal(out[~free], c["full"][~free])                       # known pixels and everything outside the window
    assert torch.equal(c["full"][~free], c["k0"][~free])
    # the control: without the margin the network sees zero padding where the full run sees the known region
    out0, (h0, w0, _, _) = _windowed(c, 0)
    assert (h0, w0) == (6, 8)
    err0 = float((out0 - c["full"])[free].abs().max())
    print(f"float64 windowed (margin 0, {h0}x{w0}) vs full keep run, free pixels: max-abs {err0:.3e}")
    assert err0 > 1e-3
    assert torch.equal(out0[~free], c["full"][~free])
    # one pixel short of the radius is not exact either: 16 is the receptive radius, not a safe guess
    out15, _ = _windowed(c, 15)
    err15 = float((out15 - c["full"])[free].abs().max())
    print(f"float64 windowed (margin 15) vs full keep run, free pixels: max-abs {err15:.3e}")
    assert err15 > 1e-12


# ---- 3: plan, refusals, parser -------------------------------------------------------------------------------------------
B3, H3, W3, T3 = 2, 48, 64, list(range(9, -1, -1))


@pytest.fixture
def model():
    net, d = build_diffusion("C2", dim=20, device="cpu")
    d.omega = 0.3
    d.img_prev_upsample = torch.zeros(B3, 3, H3, W3)
    m = torch.ones(H3, W3)
    m[20:26, 30:37] = 0
    d.keep_maps = {s: (m, torch.zeros(3, H3, W3)) for s in (0, 1)}
    return d


def test_run_plan_window_fields(model):
    d, img = model, torch.zeros(B3, 3, H3, W3)
    assert d.keep_window is None
    off = RunPlan(d, img, 1, T3)
    assert off.window is None and off.noise == ("torch", None) and off.full_hw == (H3, W3) and off.win is None
    d.keep_window = 16
    plan = RunPlan(d, img, 1, T3)
    h, w, org = plan.window
    assert (h, w) == (38, 40) and org.tolist() == [[4, 14]] * B3 and org.dtype == torch.int32
    assert plan.noise == ("window", None)                                  # unseeded: `_run_steps` draws the B seeds
    same = lambda a, b: [(x.pos, x.t, x.land, bytes(x.k), x.ab) for x in a.steps] == [(x.pos, x.t, x.land, bytes(x.k), x.ab)
                                                                                     for x in b.steps]
    assert same(plan, off) and plan.keep is not None and plan.per == off.per
    d.sample_seeds = [5, 6]
    plan = RunPlan(d, img, 1, T3)
    assert plan.noise == ("window", ([[5], [6]], None))
    assert plan.log_entry(0)[:6] == ("chain_window", 1, [5, 6], T3, None, (38, 40)) and plan.log_entry(0)[6] is plan.window[2]
    d.resample = (2, 3)
    entry = RunPlan(d, img, 1, T3).log_entry(0)
    assert entry[0] == "chain_window" and len(entry) == 7 and len(entry[3]) == len(entry[4]) > len(T3)
    d.resample, d.sample_seeds = None, None
    d.seed_mix = ([[5, 7], [6, 8]], [[0.6, 0.8], [1.0, 0.0]])
    plan = RunPlan(d, img, 1, T3)
    assert plan.noise[0] == "window" and plan.noise[1][0] == [[5, 7], [6, 8]] and plan.noise[1][1][0] == [0.6, 0.8]
    assert plan.log_entry(0)[2] == plan.noise[1]
    d.seed_mix = None
    # per-sample maps: per-sample origins; gated: the hold level < 1 is the free region
    m = torch.ones(B3, H3, W3)
    m[0, 20:26, 30:37] = 0
    m[1, 2:5, 50:60] = 0.5
    d.keep_maps = {1: (m, torch.zeros(3, H3, W3))}
    d.keep_gated = True
    plan = RunPlan(d, img, 1, T3)
    assert plan.gated and plan.window[:2] == (38, 40) and plan.window[2].tolist() == [[4, 14], [0, 24]]
    d.keep_gated = False
    # a window that spans the scale, no free pixel, a single step: today's run, field by field
    d.sample_seeds = [5, 6]
    for mask in (torch.zeros(H3, W3), torch.ones(H3, W3)):
        d.keep_maps = {1: (mask, torch.zeros(3, H3, W3))}
        plan = RunPlan(d, img, 1, T3)
        assert plan.window is None and plan.noise == ("seeds", [5, 6]) and plan.log_entry(0) == ("chain_seeds", 1, [5, 6], T3)
    d.keep_maps = {1: (m, torch.zeros(3, H3, W3))}
    assert RunPlan(d, img, 1, [5], at=(0, None, None, None)).window is None
    d.keep_window = 0
    assert RunPlan(d, img, 1, T3).window[:2] == (6, 12)


def test_run_plan_window_refusals(model, monkeypatch):
    d, img = model, torch.zeros(B3, 3, H3, W3)
    # every refusal comes before any library call: the library cannot even be loaded here
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("a library call")))
    for bad in (-1, 1.5, "16", True):
        d.keep_window = bad
        with pytest.raises(_lib.SinddmError, match="keep_window"):
            RunPlan(d, img, 1, T3)
    d.keep_window = 16
    maps, d.keep_maps = d.keep_maps, None
    with pytest.raises(_lib.SinddmError, match="keep_window without keep_maps"):
        d._run_steps(img, 1, T3)
    d.keep_maps = {0: maps[0]}
    with pytest.raises(_lib.SinddmError, match="keep_window without keep_maps"):
        RunPlan(d, img, 1, T3)                                              # no entry for the scale
    d.keep_maps = maps

    def refused(pair):
        with pytest.raises(NotImplementedError) as err:
            d._run_steps(img, 1, T3)
        assert str(err.value) == NOT_BUILT[pair]

    d.tile = (False, True)
    refused(("keep_window", "tile"))
    d.tile = (False, False)
    d.layout_maps, d.layout_down = {1: torch.zeros(3, H3, W3)}, {1: 4}
    refused(("keep_window", "layout_maps"))
    d.layout_strength = 0.0                                                # (a layout that never pulls is no layout)
    assert RunPlan(d, img, 1, T3).window is not None
    d.layout_maps, d.layout_strength = None, 1.0
    d.clip_guided_sampling = True
    refused(("keep_window", "clip"))
    d.clip_guided_sampling = False
    d.noise_fn = lambda *a: None
    refused(("keep_window", "noise_fn"))
    d.noise_fn = None
    assert RunPlan(d, img, 1, T3).window is not None
    # patch_refine with keep maps stays refused as it is
    assert ("patch_refine", "keep_maps") in NOT_BUILT


def test_keep_window_flag():
    import main
    assert main.parse_args(["--mode", "inpaint", "--mask_path", "m.png"]).keep_window is None
    assert main.parse_args(["--mode", "inpaint", "--mask_path", "m.png", "--keep_window"]).keep_window == 16
    assert main.parse_args(["--mode", "outpaint", "--keep_window", "24"]).keep_window == 24
    assert main.parse_args(["--mode", "edit", "--edit_map", "m.png", "--keep_window", "0"]).keep_window == 0
    for argv in (["--mode", "sample", "--keep_window"], ["--mode", "paint2image", "--keep_window", "16"],
                 ["--mode", "inpaint", "--mask_path", "m.png", "--keep_window", "-1"]):
        with pytest.raises(SystemExit):
            main.parse_args(argv)


def test_trainer_drivers_take_a_window():
    import inspect
    from sinddm_amd.trainer import MultiscaleTrainer
    for name in ("inpaint", "outpaint", "edit"):
        assert inspect.signature(getattr(MultiscaleTrainer, name)).parameters["window"].default is None


def test_fill_window_argument_errors():
    """Reported before any device work: safe without a GPU (the pointers are never read)."""
    lib = _lib.load()
    BADARG, BADSHAPE = -1, -2
    a8, a4 = 0x1000, 0x1004                                                # aligned to 16 / to 4 only
    ok = dict(out=a8, n=3, ids=a8, B=3, H=13, W=18, org=a8, h=6, w=7, keys=a8, wts=a8, K=1)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.sinddm_normal_fill_window(v["out"], v["n"], v["ids"], v["B"], v["H"], v["W"], v["org"], v["h"], v["w"], v["keys"],
                                             v["wts"], v["K"], None)

    for name in ("out", "ids", "org", "keys"):
        assert call(**{name: None}) == BADARG
    assert call(wts=None, K=3) == BADARG                                   # weights may be NULL only when K == 1
    for name in ("ids", "keys"):
        assert call(**{name: a4}) == BADARG                                # 8-byte tables
    for name in ("out", "org", "wts"):
        assert call(**{name: 0x1002}) == BADARG
    for name in ("n", "B", "h", "w"):
        assert call(**{name: 0}) == BADARG and call(**{name: -2}) == BADARG
    assert call(K=0) == BADARG and call(K=_lib.MIX_MAX + 1) == BADARG
    assert call(h=14) == BADSHAPE and call(w=19) == BADSHAPE
    assert call(B=65536) == BADSHAPE
    assert call(H=32768, W=32768, h=6, w=7) == BADSHAPE                    # 3 H W >= 2^31
