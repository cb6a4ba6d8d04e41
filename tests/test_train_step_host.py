"""CPU: the plan of one training step (sinddm_amd/train_step.py) -- which entries a step calls, what it refuses and when, the
cached normaliser.  No library is loaded: the plan is plain Python over the diffusion object's attributes."""
import itertools
import re

import pytest
import torch

from sinddm_amd import _lib
from sinddm_amd.autograd import l1_entry
from sinddm_amd.train_step import TrainStep

B, H, W = 2, 7, 12
TILES = {"off": (False, False), "x": (False, True), "y": (True, False), "xy": (True, True)}
L1 = {(False, False): "sinddm_l1_loss_fwd_bwd", (True, False): "sinddm_l1_loss_crop_fwd_bwd",
      (False, True): "sinddm_l1_loss_weighted_fwd_bwd", (True, True): "sinddm_l1_loss_weighted_fwd_bwd"}    # (halo, map)


@pytest.fixture
def d(monkeypatch):
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    net = SinDDMNet(dim=16, multiscale=True, device="cpu")
    d = MultiScaleGaussianDiffusion(net, n_scales=3, scale_factor=1.4, image_sizes=[(64, 48), (90, 67), (126, 94)],
                                    timesteps=20, train_full_t=True, scale_losses=[1.08, 0.77], loss_factor=1, loss_type="l1",
                                    device="cpu")

    def no_library(*a, **k):
        raise AssertionError("the plan of a training step loaded the library")

    monkeypatch.setattr(_lib, "load", no_library)
    return d


def _map():
    w = torch.linspace(0.0, 1.0, H * W).reshape(H, W).contiguous()
    w[2, 3:6] = 0.0
    return w


@pytest.mark.parametrize("tile,mask,lt,s", list(itertools.product(TILES, (False, True), ("l1", "l2", "l1_pred_img"), (0, 2))))
def test_entry_table(d, tile, mask, lt, s):
    d.train_tile, d.loss_type = TILES[tile], lt
    w = _map()
    d.train_weights = [w] * 3 if mask else None
    p = TrainStep(d, torch.Size((B, 3, H, W)), s)
    hy, hx = (16 if "y" in tile else 0), (16 if "x" in tile else 0)
    assert _lib.TILE_HALO == 16
    assert (p.s, p.loss_type, p.halo, p.shape) == (s, lt, (hy, hx), (B, 3, H, W))
    assert p.ext_shape == (B, 3, H + 2 * hy, W + 2 * hx)
    assert p.q_entry == ("sinddm_q_sample_wrap" if tile != "off" else "sinddm_q_sample")
    assert p.loss_entry == (L1[tile != "off", mask] if lt == "l1" else None)
    assert l1_entry(p.halo, mask) == L1[tile != "off", mask]                   # autograd's rule is the plan's
    if s == 0:
        assert p.gamma_row is None
    else:
        assert p.gamma_row.is_contiguous() and torch.equal(p.gamma_row, d.gammas[s - 1])     # the unclamped row
        assert float(p.gamma_row.max()) > 0.55
    if mask:
        assert p.weight is w and p.inv_norm == 1.0 / (B * 3 * float(w.to(torch.float64).sum()))
    else:
        assert p.weight is None and p.inv_norm is None


def test_refusals_by_message_and_in_order(d):
    shape = (B, 3, H, W)
    good = _map()

    def refused(maps, s, msg, exc=_lib.SinddmError):
        d.train_weights = maps
        with pytest.raises(exc, match=re.escape(msg)):
            TrainStep(d, shape, s)

    refused([good, good], 2, "train_weights holds 2 maps: none for scale 2")
    refused([good, good, torch.ones(H, W + 1)], 2, f"train_weights[2] must be a {(H, W)} fp32 tensor, got {(H, W + 1)}")
    refused([good, good, torch.ones(H, W, dtype=torch.float64)], 2, f"train_weights[2] must be a {(H, W)} fp32 tensor, got {(H, W)}")
    refused([good, None, good], 1, f"train_weights[1] must be a {(H, W)} fp32 tensor, got NoneType")
    refused([torch.zeros(H, W)], 0, "train_weights[0] sums to 0.0: scale 0 has no pixel to train on")
    bad = good.clone()
    bad[1, 1] = float("inf")
    refused([bad], 0, "train_weights[0] sums to inf: scale 0 has no pixel to train on")
    # the order: the list's length before the map, the map's form before its sum, the loss type before all of them
    refused([torch.zeros(H, W + 1)], 0, "must be a")
    refused([torch.zeros(H, W + 1)], 1, "none for scale 1")
    d.loss_type = "huber"
    for maps in (None, [torch.zeros(H, W)], []):
        d.train_weights = maps
        with pytest.raises(NotImplementedError):
            TrainStep(d, shape, 0)
    assert d._train_weight_norm == {}                                        # nothing refused was cached
    d.loss_type = "l1"
    d.train_weights = [good]
    assert TrainStep(d, shape, 0).weight is good


def test_normaliser_is_cached_per_scale_and_map_object(d):
    shape = (B, 3, H, W)
    w = _map()
    total = float(w.to(torch.float64).sum())
    d.train_weights = [w, w.clone()]
    assert TrainStep(d, shape, 0).inv_norm == 1.0 / (B * 3 * total)
    assert d._train_weight_norm[0][0] is w and d._train_weight_norm[0][1] == total and 1 not in d._train_weight_norm
    w.mul_(2.0)                                                               # in place: the same object keeps its cached sum
    assert TrainStep(d, shape, 0).inv_norm == 1.0 / (B * 3 * total)
    d.train_weights[0] = w.clone()                                            # a new object: summed again
    assert TrainStep(d, shape, 0).inv_norm == 1.0 / (B * 3 * float(w.to(torch.float64).sum())) != 1.0 / (B * 3 * total)
    assert TrainStep(d, shape, 1).inv_norm == 1.0 / (B * 3 * total)           # scale 1 has its own entry
    assert d._train_weight_norm[1][0] is d.train_weights[1]
    assert not any("train_weight" in k for k in d.state_dict())
    assert "_train_weight_norm" not in dict(d.named_buffers()) and "_train_weight_norm" in vars(d)
