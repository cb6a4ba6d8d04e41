"""CPU: tileable training (wrap-around borders in the training step) -- the construction, the command-line / trainer switches
and the two ABI additions.

The construction (tests/tile_train_util.py): extend x_noisy by a wrapped halo of SINDDM_TILE_HALO = 16 pixels, run the
ZERO-padded network on it, take the loss on the centre.  Not only the output but every parameter gradient is then the
circularly padded network's: a gradient at layer k is non-zero only within the remaining receptive radius of the centre, and
that is where the extended activations -- and so the inputs of every weight-gradient product -- are the periodic ones."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from conftest import REPO, rel_l2
from oracle import sinddm_oracle as O
from sinddm_amd import _lib
from sinddm_amd.synth import hash_randn, he_state_dict
from tile_train_util import WRAPS, autograd_in, halo_of, net_forward_circular, wrap_pad

NEW = ("sinddm_q_sample_wrap", "sinddm_l1_loss_crop_fwd_bwd")


# ---- 1: the design claim, in float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,wrap", [(5, 7, "xy"), (9, 33, "x"), (20, 12, "y"), (40, 36, "xy")])
def test_halo_training_is_circular_training_f64(H, W, wrap):
    """He-normal weights at dim 16, B = 2, float64: the circular restatement of the network against O.net_forward on the
    wrapped extension cropped to the centre -- the output and all 52 parameter gradients of the cropped L1 loss, <= 1e-12
    rel-L2 (measured: output bit-equal, gradients <= 8e-16).  5x7: the halo is wider than the image.  The zero-padded
    network's gradients are another network's (measured 2.7 % .. 95 % in every tensor): > 1e-2 in every tensor here."""
    wr = WRAPS[wrap]
    hy, hx = halo_of(wr)
    sd = he_state_dict(16)
    x = hash_randn((2, 3, H, W), 11 + H)
    target = hash_randn((2, 3, H, W), 12 + H)
    t = torch.tensor([7, 31])
    s = 2

    def halo_loss(p, x, target, out):
        y = O.net_forward(p, wrap_pad(x, hy, hx), t, s)[..., hy:hy + H, hx:hx + W]
        out.append(y.detach())
        return (target - y).abs().mean()

    def circ_loss(p, x, target, out):
        y = net_forward_circular(p, x, t, s, wr)
        out.append(y.detach())
        return (target - y).abs().mean()

    def plain_loss(p, x, target):
        return (target - O.net_forward(p, x, t, s)).abs().mean()

    ya, yb = [], []
    la, ga = autograd_in(torch.float64, lambda p, x, tg: halo_loss(p, x, tg, ya), sd, x, target)
    lb, gb = autograd_in(torch.float64, lambda p, x, tg: circ_loss(p, x, tg, yb), sd, x, target)
    lz, gz = autograd_in(torch.float64, plain_loss, sd, x, target)
    assert ya[0].dtype == torch.float64
    assert rel_l2(ya[0], yb[0]) <= 1e-12
    assert abs(float(la) - float(lb)) <= 1e-12 * abs(float(lb))
    worst = max(rel_l2(ga[k], gb[k]) for k in gb)
    apart = {k: rel_l2(gz[k], gb[k]) for k in gb}
    print(f"[{H}x{W} {wrap}] halo vs circular: output {rel_l2(ya[0], yb[0]):.1e}, worst gradient {worst:.1e}; zero-padded vs "
          f"circular gradients {min(apart.values()):.3f} .. {max(apart.values()):.3f}")
    assert len(gb) == 52
    for k in gb:
        assert rel_l2(ga[k], gb[k]) <= 1e-12, k
        assert apart[k] > 1e-2, k


# ---- 2: the switches ---------------------------------------------------------------------------------------------------------
def _pair(v):
    return ("y" in v, "x" in v)


def test_train_tile_default_and_parser():
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    import main
    net = SinDDMNet(dim=16, multiscale=True, device="cpu")
    d = MultiScaleGaussianDiffusion(net, n_scales=3, scale_factor=1.4, image_sizes=[(64, 48), (90, 67), (126, 94)],
                                    timesteps=20, train_full_t=True, scale_losses=[1.08, 0.77], loss_factor=1, loss_type="l1",
                                    device="cpu")
    assert d.train_tile == (False, False) and d.tile == (False, False)
    p = main.build_parser()
    assert p.parse_args([]).train_tile == "none"
    for v, want in (("none", (False, False)), ("x", (False, True)), ("y", (True, False)), ("xy", (True, True))):
        a = p.parse_args(["--train_tile", v])
        assert _pair(a.train_tile) == want and a.tile == "none"
    with pytest.raises(SystemExit):
        p.parse_args(["--train_tile", "z"])


ARGV = [([], (False, False), (False, False)),
        (["--train_tile", "x"], (False, True), (False, False)),
        (["--tile", "xy", "--train_tile", "y"], (True, False), (True, True)),
        (["--tile", "xy", "--train_tile", "xy"], (True, True), (True, True)),
        (["--tile", "x"], (False, False), (False, True))]


@pytest.mark.parametrize("argv,train_tile,tile", ARGV)
def test_command_line_reaches_the_trainer_call(monkeypatch, tmp_path, argv, train_tile, tile):
    """main.main() with the model, the diffusion object and the trainer replaced by recorders (main.py puts them on "cuda:0"):
    --train_tile arrives as MultiscaleTrainer(train_tile=(wrap_y, wrap_x)); the EMA copy's sampling `tile` is --tile's and
    nothing sets `tile` on the model that trains."""
    import main
    calls = []

    class Module:
        num_timesteps_ideal = [20, 10, 10]

        def __init__(self, **k):
            self.kw = k

        def to(self, device):
            return self

    class Trainer:
        def __init__(self, model, **k):
            self.model, self.ema_model, self.kw = model, Module(), k
            calls.append(self)

        def sample_scales(self, **k):
            pass

    monkeypatch.setattr(main, "MultiscaleTrainer", Trainer)
    monkeypatch.setattr(main, "SinDDMNet", Module)
    monkeypatch.setattr(main, "MultiScaleGaussianDiffusion", Module)
    monkeypatch.setattr(main, "create_img_scales", lambda *a, **k: ([(48, 64), (67, 90), (94, 126)], [1.08, 0.77], 1.4, 3))
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "sample", "--results_folder", str(tmp_path)] + argv)
    main.main()
    (tr,) = calls
    assert tr.kw["train_tile"] == train_tile
    assert tr.ema_model.tile == tile
    assert not hasattr(tr.model, "tile") and not hasattr(tr.model, "train_tile")      # (the trainer sets it, below)


@pytest.mark.parametrize("train_tile", [None, (False, True), (True, True)])
def test_trainer_sets_it_on_the_model_that_trains(golden, tmp_path, train_tile):
    """A real MultiscaleTrainer over the C1 pyramid, on the CPU: train_tile= lands on trainer.model; the EMA copy (which never
    trains) keeps the default, and both keep their sampling `tile`."""
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
    net = SinDDMNet(dim=16, multiscale=True, device="cpu")
    d = MultiScaleGaussianDiffusion(net, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"], image_sizes=sizes,
                                    timesteps=meta["T"], train_full_t=True, scale_losses=meta["rescale_losses"], loss_factor=1,
                                    loss_type="l1", device="cpu")
    kw = {} if train_tile is None else dict(train_tile=train_tile)
    tr = MultiscaleTrainer(d, folder=folder, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"], image_sizes=sizes,
                           train_batch_size=1, results_folder=str(tmp_path / "res"), device="cpu", **kw)
    assert tr.model is d
    assert tr.model.train_tile == ((False, False) if train_tile is None else train_tile)
    assert tr.ema_model.train_tile == (False, False)
    assert tr.model.tile == (False, False) and tr.ema_model.tile == (False, False)


def test_trainer_argument_default():
    """MultiscaleTrainer(train_tile=...) is optional: without it the model keeps (False, False)."""
    import inspect
    from sinddm_amd.trainer import MultiscaleTrainer
    assert inspect.signature(MultiscaleTrainer.__init__).parameters["train_tile"].default == (False, False)


# ---- 3: the ABI additions ------------------------------------------------------------------------------------------------------
def _c_params(txt, name):
    """The parameter list of `int name(...)` in the header, one C type per parameter (names dropped)."""
    body = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.S).group(1)
    out = []
    for prm in body.split(","):
        prm = " ".join(prm.split())
        out.append(re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*$", "", prm).replace(" *", "*"))
    return out


def test_abi_additions_declared_and_bound():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    lib = _lib.load()
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int64_t*": C.c_void_p, "void*": C.c_void_p,
             "int": C.c_int, "float": C.c_float}
    for name in NEW:
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        params = _c_params(txt, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [ctype[p] for p in params], (name, params)
    assert _c_params(txt, "sinddm_q_sample_wrap")[:9] == _c_params(txt, "sinddm_q_sample")[:9]      # q_sample's own arguments first
    assert int(re.search(r"#define SINDDM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 3   # symbols added, no more
    assert lib.sinddm_abi_version() == 3
    for doc in ("INTEGRATION.md",):
        body = open(os.path.join(REPO, doc)).read()
        for name in NEW:
            assert name in body, (doc, name)


def test_new_entries_reject_bad_arguments_before_any_device_work():
    lib = _lib.load()
    p = 256                                                   # a fake non-null device pointer: validation returns first
    q = lambda x0=p, nz=p, out=p, ta=p, tb=p, xo=None, gr=None, B=2, Cc=3, H=5, W=7, hy=16, hx=16: lib.sinddm_q_sample_wrap(
        x0, xo, nz, out, ta, tb, gr, None, 0, B, Cc, H, W, hy, hx, None)
    for bad in (dict(x0=None), dict(nz=None), dict(out=None), dict(ta=None), dict(tb=None), dict(xo=p), dict(B=0), dict(Cc=0),
                dict(H=0), dict(W=-3), dict(hy=-1), dict(hx=-16)):
        assert q(**bad) == -1, bad                            # SINDDM_E_BADARG
    l1 = lambda nz=p, eps=p, loss=p, BC=6, H=5, W=7, hy=16, hx=0: lib.sinddm_l1_loss_crop_fwd_bwd(nz, eps, loss, p, BC, H, W, hy,
                                                                                                 hx, 1.0, None)
    for bad in (dict(nz=None), dict(eps=None), dict(loss=None), dict(BC=0), dict(H=0), dict(W=0), dict(hy=-1), dict(hx=-1)):
        assert l1(**bad) == -1, bad
