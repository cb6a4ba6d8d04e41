"""CPU: masked training (per-pixel loss weights; holes the weights never see) -- the host helpers, the receptive-radius
statement, the ABI addition and the switches.

The statement: the network's receptive field is a square of Chebyshev radius SINDDM_TILE_HALO = 16.  A pixel
whose loss weight is 0 hands no gradient back, and a pixel further than 16 from every hole pixel computes its output -- and
every product of its backward -- from activations the hole never touched.  So with the loss switched off within 16 pixels of
the hole, the weighted loss and every parameter gradient are THE SAME NUMBERS whatever the hole contains; with one pixel less
they are not."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, rel_l2
from oracle import sinddm_oracle as O
from sinddm_amd import _lib
from sinddm_amd import functions as F
from sinddm_amd.synth import hash_randn, he_state_dict
from train_mask_util import brute_weights, radius_case, weighted_p_losses_autograd

NAME = "sinddm_l1_loss_weighted_fwd_bwd"
SIZES = [(9, 12), (18, 24), (36, 48)]


def _valid(hole):
    """(36, 48) map, 1 = train on, with the rectangle hole = (y0, y1, x0, x1) cut out."""
    v = torch.ones(SIZES[-1])
    v[hole[0]:hole[1], hole[2]:hole[3]] = 0
    return v


CORNER, INSIDE = (0, 4, 0, 6), (14, 19, 30, 33)


# ---- 1: train_weight_pyramid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hole,grow,wrap", [
    (INSIDE, 0, (False, False)), (INSIDE, 3, (False, False)), (INSIDE, [0, 3, 16], (False, False)),
    (CORNER, 3, (False, False)), (CORNER, 3, (True, True)), (CORNER, [0, 2, 16], (False, False)),
    (CORNER, [0, 2, 16], (True, True)), (CORNER, [1, 3, 16], (False, True)), (INSIDE, [1, 0, 16], (True, False))],
    ids=lambda v: str(v).replace(" ", ""))
def test_pyramid_is_the_brute_force_dilation(hole, grow, wrap):
    valid = _valid(hole)
    got = F.train_weight_pyramid(valid, SIZES, grow=grow, wrap=wrap)
    hard = F.keep_mask_pyramid(valid, SIZES, hard=True)
    grows = [grow] * len(SIZES) if isinstance(grow, int) else grow
    assert len(got) == len(SIZES)
    for s, (w, h, g) in enumerate(zip(got, hard, grows)):
        assert w.dtype == torch.float32 and tuple(w.shape) == SIZES[s]
        want = brute_weights(h.numpy(), g, wrap)
        assert np.array_equal(w.numpy(), want), (s, g)
        assert 0 < int(w.sum()) < w.numel()                                  # a hole, and something left to train on
        if g == 0:
            assert torch.equal(w, h)


def test_grow_16_everywhere_at_the_finest_size():
    """The documented setting on a single scale, both holes, against the brute force; across a wrapped border the corner hole
    takes the far edges too."""
    for hole in (CORNER, INSIDE):
        for wrap in ((False, False), (True, True)):
            valid = _valid(hole)
            (w,) = F.train_weight_pyramid(valid, SIZES[-1:], grow=16, wrap=wrap)
            assert np.array_equal(w.numpy(), brute_weights(valid.numpy(), 16, wrap)), (hole, wrap)
    (plain,) = F.train_weight_pyramid(_valid(CORNER), SIZES[-1:], grow=3)
    (wrapped,) = F.train_weight_pyramid(_valid(CORNER), SIZES[-1:], grow=3, wrap=(True, True))
    assert float(plain[-1, -1]) == 1.0 and float(wrapped[-1, -1]) == 0.0 and float(wrapped[-4, -4]) == 1.0


def test_grow_0_is_the_hard_keep_mask():
    valid = _valid(INSIDE)
    for a, b in zip(F.train_weight_pyramid(valid, SIZES), F.keep_mask_pyramid(valid, SIZES, hard=True)):
        assert torch.equal(a, b)


def test_pyramid_errors():
    valid = _valid(INSIDE)
    with pytest.raises(ValueError, match="grow"):
        F.train_weight_pyramid(valid, SIZES, grow=-1)
    with pytest.raises(ValueError, match="grow"):
        F.train_weight_pyramid(valid, SIZES, grow=[0, 0, -2])
    with pytest.raises(ValueError, match="2 grow values for 3 scales"):
        F.train_weight_pyramid(valid, SIZES, grow=[0, 1])
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        F.train_weight_pyramid(valid[None], SIZES)
    with pytest.raises(ValueError, match="scale 0 "):                        # 9x12 does not survive 16 pixels
        F.train_weight_pyramid(valid, SIZES, grow=16)
    with pytest.raises(ValueError, match="scale 1 "):
        F.train_weight_pyramid(valid, SIZES, grow=[0, 16, 16], wrap=(True, True))


# ---- 2: the fill -----------------------------------------------------------------------------------------------------------
def test_fill_mean_and_image():
    img = hash_randn((2, 3, 18, 24), 5).mul(0.5).clamp(-1, 1)
    hard = F.keep_mask_pyramid(_valid(INSIDE), SIZES, hard=True)[1]
    hole = hard < 0.5
    assert 0 < int(hole.sum()) < hole.numel()
    img[:, :, hole] = float("nan")                                           # what the hole holds must not matter
    out = F.fill_train_holes(img, hard, "mean")
    assert out.dtype == torch.float32 and out.shape == img.shape
    assert torch.equal(out[:, :, ~hole], img[:, :, ~hole])                   # the valid pixels: bit for bit
    for b in range(2):
        for c in range(3):
            mean = img[b, c][~hole].to(torch.float64).mean().to(torch.float32)
            assert torch.equal(out[b, c][hole], mean.expand(int(hole.sum())))
    clean = torch.nan_to_num(img, nan=0.25)
    same = F.fill_train_holes(clean, hard, "image")
    assert torch.equal(same, clean) and same.data_ptr() != clean.data_ptr()
    with pytest.raises(ValueError):
        F.fill_train_holes(clean, hard, "median")
    with pytest.raises(ValueError):
        F.fill_train_holes(clean, hard[:-1], "mean")


# ---- 3: the receptive radius, in float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [(False, False), (True, True)], ids=["zero-padded", "wrapped"])
def test_weights_never_see_the_hole_f64(golden, wrap):
    """grow = 16: the weighted loss and all 52 parameter gradients agree to rel-L2 <= 1e-12 between a hole of +0.9 and one of
    -0.9 (measured: exactly 0).  grow = 0: every tensor differs by more than 1e-3 (measured: 5.6e-3 at the least zero-padded,
    1.5e-2 wrapped; the losses by 2 % and 4 %).  On wrapped axes the hole grows across the border and the network is the
    circular one."""
    sched, sd, t, valid, runs = radius_case(golden, wrap)
    for grow in (16, 0):
        (w,) = F.train_weight_pyramid(valid, [(48, 64)], grow=grow, wrap=wrap)
        (la, ga), (lb, gb) = (weighted_p_losses_autograd(sched, sd, xs, xo, t, 1, nz, w, wrap) for xs, xo, nz in runs)
        diff = {k: rel_l2(ga[k], gb[k]) for k in gb}
        print(f"[{'wrapped' if any(wrap) else 'zero-padded'} grow {grow}] loss {abs(la - lb) / abs(lb):.2e}; gradients "
              f"{min(diff.values()):.2e} .. {max(diff.values()):.2e}")
        assert len(diff) == 52
        if grow == 16:
            assert abs(la - lb) <= 1e-12 * abs(lb)
            assert max(diff.values()) <= 1e-12, max(diff, key=diff.get)
        else:
            assert min(diff.values()) > 1e-3, min(diff, key=diff.get)


# ---- 4: the ABI addition ------------------------------------------------------------------------------------------------------
def test_abi_addition_declared_and_bound():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    lib = _lib.load()
    body = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.S).group(1)
    params = [re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*$", "", " ".join(p.split())).replace(" *", "*") for p in body.split(",")]
    assert params == ["const float*"] * 3 + ["float*"] * 2 + ["int"] * 6 + ["float"] * 2 + ["void*"]
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int, "float": C.c_float}
    assert NAME in _lib.ABI_SYMBOLS and hasattr(lib, NAME)
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == [ctype[p] for p in params]
    assert int(re.search(r"#define SINDDM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 3      # additive
    assert lib.sinddm_abi_version() == 3
    assert NAME in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_entry_rejects_bad_arguments_before_any_device_work():
    lib = _lib.load()
    p = 256                                                   # a fake non-null device pointer: validation returns first
    call = lambda nz=p, eps=p, w=p, loss=p, B=2, Cc=3, H=5, W=7, hy=16, hx=0, inv=0.01: getattr(lib, NAME)(
        nz, eps, w, loss, p, B, Cc, H, W, hy, hx, inv, 1.0, None)
    for bad in (dict(nz=None), dict(eps=None), dict(w=None), dict(loss=None), dict(B=0), dict(Cc=0), dict(H=0), dict(W=-2),
                dict(hy=-1), dict(hx=-16), dict(inv=0.0), dict(inv=-0.5), dict(inv=float("inf")), dict(inv=float("nan")),
                # sizes whose extended extent leaves an int, or whose element count leaves a long long
                dict(H=2 ** 31 - 1), dict(W=2 ** 30 + 1), dict(B=2 ** 31 - 1, Cc=2 ** 31 - 1, H=2 ** 30, W=2 ** 30)):
        assert call(**bad) == -1, bad                         # SINDDM_E_BADARG


# ---- 5: the switches ------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_values():
    import main
    a = main.parse_args([])
    assert a.train_mask is None and a.train_mask_grow == [0] and a.train_mask_fill == "mean"
    a = main.parse_args(["--train_mask", "hole.png", "--train_mask_grow", "0", "0", "4", "8", "16", "--train_mask_fill", "image"])
    assert a.train_mask == "hole.png" and a.train_mask_grow == [0, 0, 4, 8, 16] and a.train_mask_fill == "image"
    assert main.parse_args(["--train_mask_grow", "16"]).train_mask_grow == [16]
    for bad in (["--train_mask_fill", "median"], ["--train_mask_grow", "-1"], ["--train_mask_grow"]):
        with pytest.raises(SystemExit):
            main.parse_args(bad)
    assert "--train_mask" in main.__doc__ and "--mode inpaint --mask_path hole.png" in main.__doc__


@pytest.mark.parametrize("mode", ["train", "sample"])
def test_command_line_reaches_the_trainer_call(monkeypatch, tmp_path, mode):
    """main.main() with the model, the diffusion object and the trainer replaced by recorders: in `train` the mask file
    arrives as MultiscaleTrainer(train_mask=(H, W) {0,1} at the finest size, train_mask_grow=..., train_mask_fill=...); the
    modes that never train pass nothing, as they do nothing with --train_tile."""
    from PIL import Image
    import main
    calls = []

    class Module:
        num_timesteps_ideal = [20, 10, 10]
        image_sizes = ((64, 48), (90, 67), (126, 94))                        # (h, w), as the diffusion object holds them

        def __init__(self, **k):
            self.kw = k

        def to(self, device):
            return self

    class Trainer:
        def __init__(self, model, **k):
            self.model, self.ema_model, self.kw = model, Module(), k
            calls.append(self)

        def train(self):
            pass

        def sample_scales(self, **k):
            pass

    pic = np.full((63, 47), 255, np.uint8)                                   # half the finest size: brought to 126x94, NEAREST
    pic[10:20, 5:15] = 0
    Image.fromarray(pic).save(str(tmp_path / "hole.png"))
    monkeypatch.setattr(main, "MultiscaleTrainer", Trainer)
    monkeypatch.setattr(main, "SinDDMNet", Module)
    monkeypatch.setattr(main, "MultiScaleGaussianDiffusion", Module)
    monkeypatch.setattr(main, "create_img_scales", lambda *a, **k: ([(48, 64), (67, 90), (94, 126)], [1.08, 0.77], 1.4, 3))
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", mode, "--results_folder", str(tmp_path), "--train_mask",
                                      str(tmp_path / "hole.png"), "--train_mask_grow", "0", "4", "16"])
    main.main()
    (tr,) = calls
    if mode != "train":
        assert "train_mask" not in tr.kw
        return
    m = tr.kw["train_mask"]
    assert tuple(m.shape) == (126, 94) and m.dtype == torch.float32
    assert set(m.unique().tolist()) == {0.0, 1.0} and int((m == 0).sum()) == 400 and float(m[20:40, 10:30].sum()) == 0.0
    assert tr.kw["train_mask_grow"] == [0, 4, 16] and tr.kw["train_mask_fill"] == "mean"


def test_model_attribute_and_trainer_defaults():
    import inspect
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    from sinddm_amd.trainer import MultiscaleTrainer
    net = SinDDMNet(dim=16, multiscale=True, device="cpu")
    d = MultiScaleGaussianDiffusion(net, n_scales=3, scale_factor=1.4, image_sizes=[(64, 48), (90, 67), (126, 94)],
                                    timesteps=20, train_full_t=True, scale_losses=[1.08, 0.77], loss_factor=1, loss_type="l1",
                                    device="cpu")
    assert d.train_weights is None
    assert "train_weights" not in d.state_dict()                              # not stored in checkpoints
    prm = inspect.signature(MultiscaleTrainer.__init__).parameters
    assert (prm["train_mask"].default, prm["train_mask_grow"].default, prm["train_mask_fill"].default) == (None, 0, "mean")


@pytest.mark.parametrize("fill", ["mean", "image"])
def test_trainer_builds_the_maps_and_fills_the_holes(golden, tmp_path, fill):
    """A real MultiscaleTrainer over the C1 pyramid, on the CPU: one map per scale of that scale's size on the model that
    trains (the EMA copy keeps None), the hole pixels of both tensors of every data_list entry filled -- or left, with
    'image' -- and the valid ones untouched."""
    from PIL import Image
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    from sinddm_amd.trainer import MultiscaleTrainer
    pyr = golden("c1_pyramid.npz")
    meta = golden("g11_img_scales.json")["C1"]
    folder = str(tmp_path / "balloons") + "/"
    for key in pyr.files:
        os.makedirs(folder + key, exist_ok=True)
        Image.fromarray(pyr[key]).save(folder + key + "/balloons.png")
    sizes = [tuple(v) for v in meta["sizes"]]
    n = meta["n_scales"]

    def make(**kw):
        net = SinDDMNet(dim=16, multiscale=True, device="cpu")
        d = MultiScaleGaussianDiffusion(net, n_scales=n, scale_factor=meta["scale_factor"], image_sizes=sizes,
                                        timesteps=meta["T"], train_full_t=True, scale_losses=meta["rescale_losses"],
                                        loss_factor=1, loss_type="l1", device="cpu")
        return MultiscaleTrainer(d, folder=folder, n_scales=n, scale_factor=meta["scale_factor"], image_sizes=sizes,
                                 train_batch_size=2, results_folder=str(tmp_path / "res"), device="cpu", **kw)

    plain = make()
    assert plain.model.train_weights is None
    hw = [tuple(plain.model.image_sizes[s]) for s in range(n)]
    valid = torch.ones(hw[-1])
    valid[30:50, 20:40] = 0
    grow = [0] * (n - 1) + [3]
    tr = make(train_mask=valid, train_mask_grow=grow, train_mask_fill=fill, train_tile=(False, True))
    want = F.train_weight_pyramid(valid, hw, grow=grow, wrap=(False, True))
    hard = F.keep_mask_pyramid(valid, hw, hard=True)
    assert tr.ema_model.train_weights is None and len(tr.model.train_weights) == n
    for s in range(n):
        assert tuple(tr.model.train_weights[s].shape) == hw[s] == tuple(tr.data_list[s][0].shape[-2:])
        assert torch.equal(tr.model.train_weights[s], want[s])
        hole = hard[s] < 0.5
        assert bool(hole.any())
        for got, old in zip(tr.data_list[s], plain.data_list[s]):
            assert torch.equal(got[:, :, ~hole], old[:, :, ~hole])
            if fill == "image":
                assert torch.equal(got, old)
            else:
                assert torch.equal(got, F.fill_train_holes(old, hard[s], "mean")) and not torch.equal(got, old)
                assert bool((got[0, 0][hole] == got[0, 0][hole][0]).all())
    with pytest.raises(ValueError):
        make(train_mask=valid[:-1])
    with pytest.raises(ValueError):
        make(train_mask=valid, train_mask_fill="median")
