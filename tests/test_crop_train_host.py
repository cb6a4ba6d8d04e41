"""CPU: crop training (random windows per sample, the loss on what the network saw whole) -- the clamped draw and its coverage,
the rectangles and the normaliser, the receptive-radius statement in float64, the step plan's refusals and the switches.

The statement: with a margin of SINDDM_TILE_HALO = 16 the receptive field of a valid pixel leaves its window only
across sides that lie on the image border, where the full-image network pads with zeros too.  So the cropped step's loss and
every parameter gradient are those of full-image masked steps with the maps 1_{V_b}; with a margin of 0 they are not."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from crop_train_util import (TRIPLES, brute_norm, coverage, crop_p_losses_autograd, rect_of, statement_case,
                             statement_full_steps_f64, window_mask)
from sinddm_amd import _lib
from sinddm_amd import functions as F
from sinddm_amd.synth import hash_randn

ENTRIES = ("sinddm_q_sample_crop", "sinddm_l1_loss_rect_fwd_bwd")


# ---- H1: the clamped draw ------------------------------------------------------------------------------------------------------
def test_coverage_of_the_clamped_draw():
    """Every pixel is supervised by at least L = h - 2m and at most 3L of the draws, the minimum being exactly L; the uniform
    draw leaves the border pixel of 186 / 96 / 16 to one draw of 91, below L / 8."""
    worst = 0
    for H, h, m in TRIPLES:
        L = h - 2 * m
        hits = coverage(H, h, m)
        assert int(hits.min()) == L and int(hits.max()) <= 3 * L, (H, h, m, int(hits.min()), int(hits.max()))
        if (H, h, m) == (186, 96, 0):
            worst = int(hits.max())
    assert worst == 281
    uni = coverage(186, 96, 16, clamped=False)
    assert int(uni[0]) == int(uni[-1]) == 1 and int(uni.min()) < (96 - 32) / 8 and int(uni.max()) == 64
    assert int(uni.max()) // int(uni.min()) == 64
    uni = coverage(1024, 256, 16, clamped=False)
    assert int(uni.max()) // int(uni.min()) == 224


def test_crop_windows_draws_the_clamped_distribution():
    """In range, reproducible from a seeded generator, an uncropped axis at 0 -- and the histogram of the origins is the
    clamped one: the two end origins are drawn L times as often as an interior one."""
    g = torch.Generator().manual_seed(7)
    a = F.crop_windows(g, 4000, (50, 64), (40, 96), 16)
    assert a.dtype == torch.int64 and tuple(a.shape) == (4000, 2) and not a.is_cuda
    assert int(a[:, 0].min()) == 0 and int(a[:, 0].max()) == 10 and not bool(a[:, 1].any())
    b = F.crop_windows(torch.Generator().manual_seed(7), 4000, (50, 64), (40, 96), 16)
    assert torch.equal(a, b)
    assert not torch.equal(a, F.crop_windows(g, 4000, (50, 64), (40, 96), 16))            # (the generator moved on)
    counts = np.bincount(a[:, 0].numpy(), minlength=11)                                   # L = 8: 8 8*[1] 8 of 25 draws
    assert abs(counts[0] / 4000 - 8 / 25) < 0.03 and abs(counts[10] / 4000 - 8 / 25) < 0.03
    assert abs(counts[1:10].sum() / 4000 - 9 / 25) < 0.03
    for H, h, m in TRIPLES:
        o = F.crop_windows(g, 64, (H, 5), (h, 5), m)
        assert int(o.min()) >= 0 and int(o[:, 0].max()) <= H - h and not bool(o[:, 1].any())
    with pytest.raises(ValueError):
        F.crop_windows(g, 2, (50, 64), (32, 96), 16)                                      # L = 0


# ---- H2: rectangles and the normaliser ---------------------------------------------------------------------------------------
SIZE, CROP, M = (20, 30), (12, 14), 3
FLUSH = [(0, 5), (8, 5), (4, 0), (4, 16), (4, 5), (0, 0), (8, 16)]                        # top, bottom, left, right, none, corners


def test_crop_rects_on_every_side():
    got = F.crop_rects(torch.tensor(FLUSH), SIZE, CROP, M)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(FLUSH), 4)
    want = [(0, 9, 3, 11), (3, 12, 3, 11), (3, 9, 0, 11), (3, 9, 3, 14), (3, 9, 3, 11), (0, 9, 0, 11), (3, 12, 3, 14)]
    assert got.tolist() == [list(r) for r in want]
    assert want == [rect_of(o, SIZE, CROP, M) for o in FLUSH]
    # an axis the window spans is closed on both sides; a crop larger than the image is the image
    assert F.crop_rects(torch.tensor([(0, 7)]), SIZE, (64, 14), M).tolist() == [[0, 20, 3, 11]]
    assert F.crop_window(SIZE, (64, 14)) == (20, 14)
    assert F.crop_rects(torch.tensor([(4, 5)]), SIZE, CROP, 0).tolist() == [[0, 12, 0, 14]]


def test_crop_norm_vs_brute_force():
    win = torch.tensor(FLUSH)
    rects = F.crop_rects(win, SIZE, CROP, M)
    assert F.crop_norm(win, rects) == brute_norm(FLUSH, rects.tolist()) == float(sum((r[1] - r[0]) * (r[3] - r[2]) for r in rects.tolist()))
    wmap = hash_randn(SIZE, 31).abs().mul(0.5).clamp(0, 1)
    wmap[6:16, 7:17] = 0.0                                                    # the rectangle of origin (4, 5) lies wholly inside
    sat = F.summed_area_table(wmap)
    assert sat.dtype == torch.float64 and tuple(sat.shape) == (21, 31)
    got = F.crop_norm(win, rects, sat)
    want = brute_norm(FLUSH, rects.tolist(), wmap.numpy())
    assert abs(got - want) <= 1e-12 * want
    assert F.crop_norm(win[4:5], rects[4:5], sat) == 0.0 == brute_norm(FLUSH[4:5], rects[4:5].tolist(), wmap.numpy())
    empty = torch.tensor([[3, 3, 0, 5]])
    assert F.crop_norm(win[:1], empty, sat) == 0.0 and F.crop_norm(win[:1], empty) == 0.0


# ---- H3: the statement, in float64 -------------------------------------------------------------------------------------------
def test_crop_step_is_a_masked_full_image_step_f64(golden):
    """margin 16: the crop loss and all 52 parameter gradients equal the area-weighted combination of the two full-image masked
    steps to rel-L2 <= 1e-12 (tests/test_train_mask_host.py's bound for two float64 results that are the same numbers).
    margin 0: the worst tensor is more than 1e-2 away."""
    case = statement_case(golden)
    for m in (16, 0):
        rects = [rect_of(o, case["size"], case["window"], m) for o in case["windows"]]
        mask = window_mask(2, case["window"], rects)
        l_crop, g_crop = crop_p_losses_autograd(case["sched"], case["sd"], case["x_start"], case["x_orig"], case["t"], 1,
                                                case["noise"], mask, case["windows"])
        l_full, g_full = statement_full_steps_f64(case, m)
        diff = {k: rel_l2(g_crop[k], g_full[k]) for k in g_full}
        print(f"[margin {m}] loss {abs(l_crop - l_full) / abs(l_full):.2e}; gradients {min(diff.values()):.2e} .. "
              f"{max(diff.values()):.2e}")
        assert len(diff) == 52
        if m == 16:
            assert abs(l_crop - l_full) <= 1e-12 * abs(l_full)
            assert max(diff.values()) <= 1e-12, max(diff, key=diff.get)
        else:
            assert max(diff.values()) > 1e-2


# ---- H4: the step plan ----------------------------------------------------------------------------------------------------------
def _diffusion():
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    net = SinDDMNet(dim=16, multiscale=True, device="cpu")
    return MultiScaleGaussianDiffusion(net, n_scales=3, scale_factor=1.4, image_sizes=[(64, 48), (90, 67), (126, 94)],
                                       timesteps=20, train_full_t=True, scale_losses=[1.08, 0.77], loss_factor=1, loss_type="l1",
                                       device="cpu")


def _no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a library entry was called by the step plan")
    lib = _lib.load()
    for name in _lib.ABI_SYMBOLS:
        if name.startswith(("sinddm_q_sample", "sinddm_l1_loss", "sinddm_net_")):
            monkeypatch.setattr(lib, name, refuse)


def test_plan_of_a_cropped_and_of_an_uncropped_scale(monkeypatch):
    from sinddm_amd.train_step import TrainStep
    _no_library(monkeypatch)
    d = _diffusion()
    assert d.train_crop is None and d.train_crop_margin == 0 and d.crop_fn is None
    assert "train_crop" not in d.state_dict()
    d.train_crop, d.train_crop_margin = (48, 64), 16
    plan = TrainStep(d, (2, 3, 48, 64), 0)                                   # not larger than the crop: today's plan
    assert plan.crop is None and plan.windows is None and plan.rects is None and plan.inv_norm is None
    assert (plan.q_entry, plan.loss_entry, plan.ext_shape) == ("sinddm_q_sample", "sinddm_l1_loss_fwd_bwd", (2, 3, 48, 64))
    plan = TrainStep(d, (2, 3, 67, 90), 1, windows=torch.tensor([[0, 5], [19, 26]]))
    assert plan.crop == (48, 64) and plan.ext_shape == (2, 3, 48, 64)
    assert (plan.q_entry, plan.loss_entry) == ENTRIES
    assert plan.windows.dtype == plan.rects.dtype == torch.int32
    assert plan.windows.tolist() == [[0, 5], [19, 26]] and plan.rects.tolist() == [[0, 32, 16, 48], [16, 48, 16, 64]]
    assert plan.inv_norm == 1.0 / (3 * (32 * 32 + 32 * 48))
    win, rects = plan.tables("cpu")
    assert torch.equal(win, plan.windows) and torch.equal(rects, plan.rects)
    calls = []
    plan = TrainStep(d, (2, 3, 67, 90), 1, draw=lambda: calls.append(1) or torch.tensor([[3, 3], [4, 4]]))
    assert len(calls) == 1 and plan.windows.tolist() == [[3, 3], [4, 4]]
    d.loss_type = "l2"
    assert TrainStep(d, (2, 3, 67, 90), 1, windows=[[0, 0], [1, 1]]).loss_entry is None


def test_plan_refusals_before_any_library_call(monkeypatch):
    from sinddm_amd.train_step import CROP_REDRAWS, TrainStep
    _no_library(monkeypatch)
    d = _diffusion()
    win = torch.tensor([[0, 5], [19, 26]])
    d.train_crop, d.train_crop_margin = (48, 64), 24                         # a 48-pixel window is not larger than 2 * 24
    with pytest.raises(_lib.SinddmError, match="two margins"):
        TrainStep(d, (2, 3, 67, 90), 1, windows=win)
    TrainStep(d, (2, 3, 48, 64), 0)                                          # (an uncropped scale does not care)
    d.train_crop_margin = 16
    d.train_tile = (False, True)
    with pytest.raises(_lib.SinddmError, match="train_tile"):
        TrainStep(d, (2, 3, 67, 90), 1, windows=win)
    with pytest.raises(_lib.SinddmError, match="train_tile"):
        TrainStep(d, (2, 3, 48, 64), 0)                                      # whatever the scale
    d.train_tile = (False, False)
    for bad in (torch.tensor([[0, 5], [20, 26]]), torch.tensor([[0, 5], [19, 27]]), torch.tensor([[-1, 5], [19, 26]]),
                torch.tensor([[0, 5]]), torch.tensor([[0.0, 5.0], [19.0, 26.0]])):
        with pytest.raises(_lib.SinddmError, match="origins"):
            TrainStep(d, (2, 3, 67, 90), 1, windows=bad)
    with pytest.raises(_lib.SinddmError, match="neither windows nor a draw"):
        TrainStep(d, (2, 3, 67, 90), 1)
    for crop, m in (((48,), 0), ((0, 64), 0), ((48, 64), -1), ("ab", 0)):
        d.train_crop, d.train_crop_margin = crop, m
        with pytest.raises(_lib.SinddmError, match="train_crop"):
            TrainStep(d, (2, 3, 67, 90), 1, windows=win)
    # a batch whose valid rectangles hold no weight: explicit windows at once, a draw after 1 + CROP_REDRAWS tries
    d.train_crop, d.train_crop_margin = (48, 64), 16
    wmap = torch.ones(67, 90)
    wmap[:, 21:] = 0
    d.train_weights = [None, wmap, None]
    with pytest.raises(_lib.SinddmError, match="no weight"):
        TrainStep(d, (2, 3, 67, 90), 1, windows=win)
    calls = []
    with pytest.raises(_lib.SinddmError, match="no weight"):
        TrainStep(d, (2, 3, 67, 90), 1, draw=lambda: calls.append(1) or win)
    assert len(calls) == 1 + CROP_REDRAWS == 17
    seq = iter([win, win, torch.tensor([[0, 0], [19, 26]])])                 # the third draw sees the map's top-left corner
    plan = TrainStep(d, (2, 3, 67, 90), 1, draw=lambda: next(seq))
    assert plan.windows.tolist() == [[0, 0], [19, 26]] and plan.inv_norm == 1.0 / (3 * 32.0 * 21)
    assert d._train_crop_sat[1][0] is wmap


def test_p_losses_draws_windows_and_honours_crop_fn(monkeypatch):
    """p_losses hands TrainStep the explicit windows, else crop_fn(crop_step, s, B), else the clamped draw from the private
    generator (seeded from torch.initial_seed(): two objects draw the same windows)."""
    from sinddm_amd import models
    seen = []

    class Stop(Exception):
        pass

    def plan(d, shape, s, windows=None, draw=None):
        seen.append(windows if windows is not None else draw())
        raise Stop

    monkeypatch.setattr(models, "TrainStep", plan)
    x, t = torch.zeros(2, 3, 67, 90), torch.zeros(2, dtype=torch.long)
    torch.manual_seed(5)
    for d in (_diffusion(), _diffusion()):
        d.train_crop, d.train_crop_margin = (48, 64), 16
        for _ in range(2):
            with pytest.raises(Stop):
                d.p_losses(x, t, 1)
    assert torch.equal(seen[0], seen[2]) and torch.equal(seen[1], seen[3]) and not torch.equal(seen[0], seen[1])
    assert tuple(seen[0].shape) == (2, 2) and int(seen[0][:, 0].max()) <= 19 and int(seen[0][:, 1].max()) <= 26
    d.crop_fn, d.crop_step = (lambda step, s, B: torch.tensor([[step, s]] * B)), 9
    with pytest.raises(Stop):
        d.p_losses(x, t, 1)
    assert seen[-1].tolist() == [[9, 1], [9, 1]]
    with pytest.raises(Stop):
        d.p_losses(x, t, 1, windows=[[1, 2], [3, 4]])
    assert seen[-1] == [[1, 2], [3, 4]]


# ---- the ABI additions and the switches -----------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_before_any_device_work():
    lib = _lib.load()
    p = 256                                                   # a fake non-null device pointer: validation returns first
    q = lambda x0=p, xo=None, nz=p, out=p, ta=p, tb=p, gam=None, win=p, B=2, Cc=3, H=9, W=13, h=5, w=6: lib.sinddm_q_sample_crop(
        x0, xo, nz, out, ta, tb, gam, None, 0, win, B, Cc, H, W, h, w, None)
    for bad in (dict(x0=None), dict(nz=None), dict(out=None), dict(ta=None), dict(tb=None), dict(win=None), dict(xo=p),
                dict(B=0), dict(Cc=0), dict(H=0), dict(W=-1), dict(h=0), dict(w=0), dict(h=10), dict(w=14),
                dict(Cc=2 ** 10, H=2 ** 10, W=2 ** 10, h=5, w=6)):
        assert q(**bad) == -1, bad
    l = lambda nz=p, eps=p, wt=None, win=None, rect=p, loss=p, B=2, Cc=3, h=5, w=6, Hm=0, Wm=0, inv=0.01: \
        lib.sinddm_l1_loss_rect_fwd_bwd(nz, eps, wt, win, rect, loss, p, B, Cc, h, w, Hm, Wm, inv, 1.0, None)
    for bad in (dict(nz=None), dict(eps=None), dict(rect=None), dict(loss=None), dict(B=0), dict(Cc=0), dict(h=0),
                dict(w=-2), dict(inv=0.0), dict(inv=-0.5), dict(inv=float("inf")), dict(inv=float("nan")),
                dict(wt=p, win=None, Hm=9, Wm=13), dict(wt=p, win=p, Hm=4, Wm=13), dict(wt=p, win=p, Hm=9, Wm=5),
                dict(wt=p, win=p, Hm=0, Wm=0), dict(h=2 ** 30 + 1), dict(B=2 ** 31 - 1, Cc=2 ** 31 - 1, h=2 ** 30, w=2 ** 30)):
        assert l(**bad) == -1, bad
    assert all(n in _lib.ABI_SYMBOLS and hasattr(lib, n) for n in ENTRIES) and lib.sinddm_abi_version() == 3


def test_l1_entry_is_unchanged_for_existing_arguments():
    from sinddm_amd.autograd import l1_entry
    assert l1_entry((0, 0), False) == "sinddm_l1_loss_fwd_bwd" and l1_entry((16, 0), False) == "sinddm_l1_loss_crop_fwd_bwd"
    assert l1_entry((0, 0), True) == l1_entry((0, 16), True) == "sinddm_l1_loss_weighted_fwd_bwd"
    assert l1_entry((0, 0), False, True) == l1_entry((0, 0), True, True) == "sinddm_l1_loss_rect_fwd_bwd"


def test_parser_and_trainer_defaults():
    import inspect
    import main
    from sinddm_amd.trainer import MultiscaleTrainer
    a = main.parse_args([])
    assert a.train_crop is None and a.train_crop_margin == 0
    a = main.parse_args(["--train_crop", "96", "128", "--train_crop_margin", "16"])
    assert a.train_crop == [96, 128] and a.train_crop_margin == 16
    for bad in (["--train_crop", "96", "96", "--train_tile", "x"], ["--train_crop", "96", "96", "--train_tile", "xy"],
                ["--train_crop", "96"], ["--train_crop", "0", "96"], ["--train_crop_margin", "-1"]):
        with pytest.raises(SystemExit):
            main.parse_args(bad)
    assert "--train_crop H W" in main.__doc__
    prm = inspect.signature(MultiscaleTrainer.__init__).parameters
    assert (prm["train_crop"].default, prm["train_crop_margin"].default) == (None, 0)
