"""CPU: tileable sampling (wrap-around borders per axis) -- the construction, the ABI additions, argument validation and
the Python / command-line switches.

The construction: SinDDMNet's receptive radius is 16 pixels (per block depthwise 5x5 (2) + 3x3 (1) + 3x3 (1) = 4; four
blocks; the 1x1 convolutions add nothing), so the ZERO-padded network on an image extended by a 16-pixel wrapped halo
equals, on the centre, the network with circular padding in every layer.  No convolution kernel is touched."""
import ctypes as C
import os
import re

import torch

from conftest import REPO, rel_l2
from oracle import sinddm_oracle as O
from sinddm_amd import _lib
from sinddm_amd.synth import closed_form_state_dict, hash_randn
from tile_util import HALO, centre, circular_oracle, wrap_pad

NEW = ("sinddm_wrap_halo", "sinddm_upsample_bilinear_wrap", "sinddm_sample_chain_tile")


def _halo_net(sd, x, t, s, hy, hx):
    return centre(O.net_forward(sd, wrap_pad(x, hy, hx), t, s), hy, hx)


def test_halo_16_is_the_circular_network_and_15_is_not():
    """dim 16, closed-form weights, B = 2, 17x19.  "Equal" is 1e-6 rel-L2: the same sums in fp32, possibly evaluated by
    another CPU convolution routine for the larger shape (measured: 0.0).  Halo 15 lets the zero padding reach the
    outermost centre pixels through the full 16-pixel receptive radius: measured 1.8e-5."""
    sd = closed_form_state_dict(16)
    x = hash_randn((2, 3, 17, 19), 5)
    t = torch.tensor([7, 7], dtype=torch.long)
    with torch.no_grad():
        plain = O.net_forward(sd, x, t, 1)
        with circular_oracle((True, True)):
            circ = O.net_forward(sd, x, t, 1)
            circ_rolled = O.net_forward(sd, torch.roll(x, (5, 7), (2, 3)), t, 1)
        assert torch.equal(plain, O.net_forward(sd, x, t, 1))              # the patch is gone after the block
        errs = {h: rel_l2(_halo_net(sd, x, t, 1, h, h), circ) for h in (HALO, HALO - 1, 12)}
        print("halo vs circular oracle, rel-L2:", {h: "%.2e" % e for h, e in errs.items()},
              "zero-pad net vs circular: %.2e" % rel_l2(plain, circ))
        assert errs[HALO] <= 1e-6
        assert errs[HALO - 1] > 3e-6 and errs[12] > errs[HALO - 1]
        assert rel_l2(plain, circ) > 0.1                                    # another network, not a rounding difference
        # the circular network commutes with toroidal shifts; the zero-padded one does not
        assert rel_l2(circ_rolled, torch.roll(circ, (5, 7), (2, 3))) <= 1e-6
        assert rel_l2(O.net_forward(sd, torch.roll(x, (5, 7), (2, 3)), t, 1), torch.roll(plain, (5, 7), (2, 3))) > 0.1
        # the axes are independent: a halo on one axis = circular on that axis, zero padding on the other
        for wrap in ((False, True), (True, False)):
            with circular_oracle(wrap):
                ref = O.net_forward(sd, x, t, 1)
            hy, hx = (HALO if wrap[0] else 0), (HALO if wrap[1] else 0)
            assert rel_l2(_halo_net(sd, x, t, 1, hy, hx), ref) <= 1e-6, wrap
            assert rel_l2(ref, circ) > 0.1 and rel_l2(ref, plain) > 0.1


def test_abi_additions():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.ABI_SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert int(re.search(r"#define SINDDM_TILE_HALO (\d+)", txt).group(1)) == _lib.TILE_HALO == 16
    assert int(re.search(r"#define SINDDM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 3     # symbols added, no more
    assert lib.sinddm_abi_version() == 3


def test_arguments_are_rejected_before_any_device_work():
    lib = _lib.load()
    one = C.cast(C.pointer(_lib.StepCoefs()), C.POINTER(_lib.StepCoefs))
    tl = (C.c_int * 1)(0)
    flag = C.c_int(7)

    def chain(hy, hx):
        # (fake non-null device pointers: validation returns before anything is enqueued or dereferenced)
        return lib.sinddm_sample_chain_tile(256, 256, 256, 256, 256, None, one, tl, 1, 0.0, 1, 0, 160, 1, 8, 8, 256, 0, None,
                                            None, C.byref(flag), None, hy, hx)

    assert chain(5, 0) == -1 and chain(0, 5) == -1 and chain(5, 5) == -1          # SINDDM_E_BADARG
    assert chain(_lib.TILE_HALO - 1, _lib.TILE_HALO) == -1 and chain(-16, 0) == -1
    # accepted halos: the (empty) workspace is what fails next
    assert chain(0, 0) == -3 and chain(_lib.TILE_HALO, 0) == -3 and chain(_lib.TILE_HALO, 24) == -3
    assert flag.value == 7
    assert lib.sinddm_wrap_halo(None, None, 6, 17, 19, 16, 16, None) == -1
    assert lib.sinddm_wrap_halo(None, 256, 6, 17, 19, 16, 16, None) == -1
    assert lib.sinddm_wrap_halo(256, None, 6, 17, 19, -1, 16, None) == -1
    assert lib.sinddm_wrap_halo(256, None, 0, 17, 19, 16, 16, None) == -1
    assert lib.sinddm_upsample_bilinear_wrap(None, None, 1, 2, 2, 4, 4, 1, 1, None) == -1


def test_tile_defaults_and_command_line():
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    net = SinDDMNet(dim=16, multiscale=True, device="cpu")
    d = MultiScaleGaussianDiffusion(net, n_scales=3, scale_factor=1.4, image_sizes=[(64, 48), (90, 67), (126, 94)],
                                    timesteps=20, train_full_t=True, scale_losses=[1.08, 0.77], loss_factor=1, loss_type="l1",
                                    device="cpu")
    assert d.tile == (False, False)
    assert d._tile_halo() == (0, 0)
    d.tile = (False, True)
    assert d._tile_halo() == (0, _lib.TILE_HALO)
    import main
    p = main.build_parser()
    assert p.parse_args([]).tile == "none"
    assert p.parse_args(["--tile", "xy"]).tile == "xy"
    for v, want in (("none", (False, False)), ("x", (False, True)), ("y", (True, False)), ("xy", (True, True))):
        t = p.parse_args(["--tile", v]).tile
        assert ("y" in t, "x" in t) == want
