"""CPU: the host side of the denoising score (sinddm_amd/score.py, MultiScaleGaussianDiffusion.denoise_score's checks, the
command line) and the float64 restatement the GPU tests compare against (tests/score_util.py).  No device; the argument checks
run with the library stubbed out, so they are shown to come before any library call.
reference: none (the score is this project's own instrument; its quantity is the reference's training loss, models.py:578-611)"""
import os

import numpy as np
import pytest
import torch

from sinddm_amd import _lib
from sinddm_amd.models import noise_stream_id
from sinddm_amd.score import (SCORE_STREAM, SCORE_STREAM_END, score_edit_map, score_levels, score_pyramid, score_stream_id)


# ---- score_levels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(100, 10), (100, 7), (1000, 10), (522, 3), (20, 20), (5, 2), (228, 64)])
def test_levels_cover_the_range(T, n):
    lv = score_levels(T, n)
    assert len(lv) == n and lv[0] == 0 and lv[-1] == T - 1
    assert all(b > a for a, b in zip(lv, lv[1:]))
    assert all(isinstance(t, int) for t in lv)


def test_levels_clip_and_refuse():
    assert score_levels(5, 9) == [0, 1, 2, 3, 4]                 # n > T: every level, once
    assert score_levels(1, 3) == [0]
    assert score_levels(100, 1) == [49]
    assert score_levels(100, 10) == list(range(0, 100, 11))      # evenly spaced: one cond_kernel launch in the library
    for T, n in ((0, 3), (10, 0), (10, -1)):
        with pytest.raises(ValueError):
            score_levels(T, n)


# ---- score_edit_map ----------------------------------------------------------------------------------------------------------
def test_edit_map_range_and_monotone():
    g = torch.Generator().manual_seed(5)
    train = torch.rand(23, 31, generator=g) * 3.0 + 0.5
    img = torch.rand(23, 31, generator=g) * 6.0
    e = score_edit_map(img, train)
    assert e.dtype == torch.float32 and tuple(e.shape) == (23, 31)
    assert float(e.min()) >= 0.0 and float(e.max()) <= 1.0
    assert float(e.min()) == 0.0 and float(e.max()) == 1.0       # (this picture goes below the median and above the maximum)
    order = img.flatten().argsort()
    assert bool((e.flatten()[order].diff() >= 0).all())          # monotone in the score
    # the training image against itself: <= 1 everywhere, 1 at its maximum, 0 at its median and below
    own = score_edit_map(train, train)
    m = train.flatten().median()
    assert float(own.max()) == 1.0 and float(own.flatten()[train.flatten().argmax()]) == 1.0
    assert bool((own[train <= m] == 0).all()) and bool((own[train > m] > 0).all())
    assert abs(float((own == 0).float().mean()) - 0.5) < 0.01


def test_edit_map_flat_and_defective_training_map():
    flat = torch.full((4, 4), 2.0)
    e = score_edit_map(torch.tensor([[1.0, 2.0], [3.0, 2.5]]), flat)
    assert e.tolist() == [[0.0, 0.0], [1.0, 1.0]]
    with pytest.raises(ValueError):
        score_edit_map(torch.zeros(2, 2), torch.tensor([[1.0, float("nan")]]))
    with pytest.raises(ValueError):
        score_edit_map(torch.zeros(2, 2), torch.zeros(0))


def test_edit_map_leaves_holes_out_of_the_normalisation():
    """Under a weight plane the holes of a score map are exact zeros: with `valid` the median and the maximum are those of the
    valid pixels, the map equals the one computed from the valid pixels alone, and a hole of the picture's map comes out 0."""
    g = torch.Generator().manual_seed(9)
    train = torch.rand(20, 30, generator=g) + 1.0
    img = torch.rand(20, 30, generator=g) * 3.0
    valid = torch.ones(20, 30, dtype=torch.bool)
    valid[:12] = False                                                           # more than half the plane is a hole
    train_h, img_h = train * valid, img * valid
    e = score_edit_map(img_h, train_h, valid=valid)
    want = score_edit_map(img[valid], train[valid])
    assert torch.equal(e[valid], want) and float(e[~valid].abs().max()) == 0.0
    naive = score_edit_map(img_h, train_h)                                       # the zeros would drag the median to 0
    assert not torch.equal(naive[valid], want)
    with pytest.raises(ValueError):
        score_edit_map(img_h, train_h, valid=torch.ones(20, 29))
    with pytest.raises(ValueError):
        score_edit_map(img_h, train_h, valid=torch.zeros(20, 30))


# ---- stream ids --------------------------------------------------------------------------------------------------------------
def test_stream_ids_do_not_meet_the_samplers():
    assert SCORE_STREAM == 0x40000000 and SCORE_STREAM_END == _lib.JUMP_STREAM
    for s in (0, 1, 7):
        lo, hi = score_stream_id(s, 0), score_stream_id(s, SCORE_STREAM_END - SCORE_STREAM - 1)
        assert lo == (s << 32) | 0x40000000 and hi == (s << 32) | 0x7fffffff
        sampler = [noise_stream_id(s, "init"), noise_stream_id(s, "renoise")]
        # a scale's run is at most a few thousand steps, resampling included; a million positions is far past any of them
        sampler += [noise_stream_id(s, "step", i) for i in (0, 1, 999, 10 ** 6)]
        sampler += [noise_stream_id(s, "jump", i) for i in (0, 1, 999, 10 ** 6)]
        assert all(not lo <= k <= hi for k in sampler)
        assert max(k for k in sampler if k < lo) == noise_stream_id(s, "step", 10 ** 6)
        assert min(k for k in sampler if k > hi) == noise_stream_id(s, "jump", 0)
        # and the ranges of two scales are disjoint
        assert hi < score_stream_id(s + 1, 0)
    assert [score_stream_id(2, i) - score_stream_id(2, 0) for i in range(4)] == [0, 1, 2, 3]
    for bad in ((-1, 0), (0, -1), (0, SCORE_STREAM_END - SCORE_STREAM), (1 << 31, 0)):
        with pytest.raises(ValueError):
            score_stream_id(*bad)


# ---- score_pyramid -----------------------------------------------------------------------------------------------------------
def test_pyramid_shapes_and_partners():
    sizes = [(12, 16), (17, 23), (24, 32)]
    up = lambda t, size: torch.nn.functional.interpolate(t, size=size, mode="bilinear", align_corners=False)
    pic = torch.linspace(-1, 1, 3 * 24 * 32).reshape(3, 24, 32)
    pyr = score_pyramid(pic, sizes, upsample=up)
    assert len(pyr) == 3 and pyr[0][1] is None
    for s, (y, yp) in enumerate(pyr):
        assert tuple(y.shape) == (1, 3) + sizes[s] and y.dtype == torch.float32
        if s > 0:
            assert tuple(yp.shape) == tuple(y.shape)
            assert torch.equal(yp, up(pyr[s - 1][0], sizes[s]))                  # the scale below, upsampled
    assert torch.equal(pyr[2][0][0], pic)                                        # the finest scale is the picture
    const = score_pyramid(torch.full((2, 3, 24, 32), 0.25), sizes, upsample=up)
    for y, yp in const:
        assert tuple(y.shape)[0] == 2 and float((y - 0.25).abs().max()) < 1e-6
    with pytest.raises(ValueError):
        score_pyramid(torch.zeros(3, 20, 32), sizes, upsample=up)                # not the finest size
    with pytest.raises(ValueError):
        score_pyramid(torch.zeros(24, 32), sizes, upsample=up)


# ---- denoise_score: every refusal comes before the library ---------------------------------------------------------------------
@pytest.fixture
def d(monkeypatch):
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    net = SinDDMNet(dim=16, multiscale=True, device="cpu")
    d = MultiScaleGaussianDiffusion(net, n_scales=3, scale_factor=1.4, image_sizes=[(64, 48), (90, 67), (126, 94)],
                                    timesteps=20, train_full_t=True, scale_losses=[1.08, 0.77], loss_factor=1, loss_type="l1",
                                    device="cpu")

    def no_library(*a, **k):
        raise AssertionError("denoise_score reached the library with arguments it must refuse")

    monkeypatch.setattr(_lib, "load", no_library)
    return d


def test_denoise_score_refusals(d):
    y = torch.zeros(2, 3, 12, 16)
    yp = torch.zeros(2, 3, 12, 16)
    bad = [
        (dict(y=y, s=0, levels=[0, 20]), ValueError),                                # a level the scale was not trained on
        (dict(y=y, s=0, levels=[-1]), ValueError),
        (dict(y=y, s=0, levels=[]), ValueError),
        (dict(y=y, s=3), ValueError),                                                # no such scale
        (dict(y=y, s=0, y_prev=yp), ValueError),                                     # scale 0 has no blurred image
        (dict(y=y, s=2), ValueError),                                                # ... and a finer scale needs one
        (dict(y=y, s=1, y_prev=torch.zeros(2, 3, 12, 15)), ValueError),              # shape mismatches
        (dict(y=y, s=1, y_prev=torch.zeros(1, 3, 12, 16)), ValueError),
        (dict(y=torch.zeros(3, 12, 16), s=0), ValueError),
        (dict(y=torch.zeros(2, 1, 12, 16), s=0), ValueError),
        (dict(y=y.double(), s=0), ValueError),
        (dict(y=y, s=0, weight=torch.ones(12, 15)), ValueError),
        (dict(y=y, s=0, weight=torch.ones(2, 12, 16)), ValueError),                  # per-sample planes are not built
        (dict(y=y, s=0, weight=torch.zeros(12, 16)), ValueError),                    # nothing to score, no mean over sum(w)
        (dict(y=y, s=0, weight=torch.ones(12, 16).index_put((torch.tensor(3), torch.tensor(4)), torch.tensor(-1.0))), ValueError),
        (dict(y=y, s=0, weight=torch.ones(12, 16).index_put((torch.tensor(3), torch.tensor(4)), torch.tensor(float("nan")))),
         ValueError),
        (dict(y=y, s=0, weight=torch.full((12, 16), float("inf"))), ValueError),
        (dict(y=y, s=0, draws=0), ValueError),
        (dict(y=y, s=0, draws=2, seeds=[1, 2]), ValueError),                         # B * draws seeds
        (dict(y=y, s=0, seeds=[1, 1 << 63]), ValueError),
    ]
    for kw, exc in bad:
        with pytest.raises(exc):
            d.denoise_score(**kw)
    for tile in ((True, False), (False, True), (True, True)):
        d.tile = tile
        with pytest.raises(NotImplementedError):
            d.denoise_score(y, 0)
    d.tile = (False, False)
    # a good call gets as far as the library: the stub is what stops it
    with pytest.raises(AssertionError, match="reached the library"):
        d.denoise_score(y, 1, y_prev=yp, levels=[0, 19], draws=2, seeds=[1, 2, 3, 4], weight=torch.ones(12, 16))


def test_sampler_not_built_is_untouched():
    """The score adds no sampling option: sampler.NOT_BUILT keeps its entries."""
    from sinddm_amd import sampler
    assert not any("score" in str(k).lower() for k in sampler.NOT_BUILT)


# ---- the binding and the entry's refusals that need no device ---------------------------------------------------------------------
def test_entry_refuses_before_any_device_work():
    lib = _lib.load()
    assert _lib.SCORE_MAX_EVALS == 1024
    assert lib.sinddm_score_workspace_bytes(16, 2, 12, 16, 0) == 0
    assert lib.sinddm_score_workspace_bytes(16, 2, 12, 16, 1025) == 0
    assert lib.sinddm_score_workspace_bytes(16, 0, 12, 16, 3) == 0
    assert lib.sinddm_score_workspace_bytes(3, 2, 12, 16, 3) == 0
    for dim, B, H, W in ((16, 2, 12, 16), (16, 3, 13, 17), (20, 2, 13, 17), (160, 16, 67, 90)):
        a, b = lib.sinddm_score_workspace_bytes(dim, B, H, W, 1), lib.sinddm_score_workspace_bytes(dim, B, H, W, 1024)
        assert lib.sinddm_workspace_bytes(dim, B, H, W) <= a <= b
    # dim 20 at 13x17 has no fused tail: one eps tensor rides behind the partials
    assert (lib.sinddm_score_workspace_bytes(20, 2, 13, 17, 1) - lib.sinddm_workspace_bytes(20, 2, 13, 17)
            >= 2 * 3 * 13 * 17 * 4)
    assert lib.sinddm_score_chain(None, None, None, None, None, None, None, None, None, 1, 0.0, 0, 0, None, None, 16, 1, 8, 8,
                                  None, 0, None, None) == -1


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------
def test_restatement_is_the_oracles_training_loss(golden):
    """score_util.score_f64 with one level, no weight: sum(level) / (B 3 HW) is O.p_losses ('l1') of the same inputs, and the
    map's sum is the level."""
    from oracle import sinddm_oracle as O
    from score_util import level_sum_f64, score_f64
    from sinddm_amd.synth import hash_randn, he_state_dict
    meta = golden("g11_img_scales.json")["C1"]
    sched = O.make_schedule(meta["T"], meta["n_scales"], meta["rescale_losses"], 1, train_full_t=True)
    sd = he_state_dict(16)
    B, H, W = 2, 9, 11
    y = hash_randn((B, 3, H, W), 1).mul(0.5).clamp(-1, 1)
    yp = hash_randn((B, 3, H, W), 2).mul(0.5).clamp(-1, 1)
    z = hash_randn((1, B, 3, H, W), 3)
    for s, t in ((0, 40), (2, 17)):
        smap, level = score_f64(sched, sd, y, yp if s else None, s, [t], z)
        tt = torch.full((B,), t, dtype=torch.long)
        want = float(O.p_losses(sched, sd, yp if s else y, tt, s, z[0], x_orig=y if s else None))
        got = float(level.sum()) / (B * 3 * H * W)
        assert abs(got - want) <= 2e-5 * abs(want), (s, got, want)              # (the oracle's network runs in fp32)
        assert np.allclose(smap.sum(dim=(1, 2)).numpy(), level[0].numpy(), rtol=1e-12)
        assert np.allclose(level_sum_f64(smap.float().numpy()), level[0].numpy(), rtol=1e-6)
    # a weight plane with zeros: the pixels are 0 in the map and absent from the level
    w = torch.ones(H, W)
    w[:, :4] = 0
    smap, level = score_f64(sched, sd, y, None, 0, [40], z, weight=w)
    full, _ = score_f64(sched, sd, y, None, 0, [40], z)
    assert float(smap[:, :, :4].abs().max()) == 0.0 and torch.equal(smap[:, :, 4:], full[:, :, 4:])
    assert np.allclose(level[0].numpy(), full[:, :, 4:].sum(dim=(1, 2)).numpy(), rtol=1e-12)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_command_line_accepts_score():
    import main
    p = main.build_parser()
    a = p.parse_args(["--mode", "score", "--score_levels", "7", "--score_draws", "3", "--score_scales", "1", "2",
                      "--input_image", "a.png", "b.png"])
    assert (a.mode, a.score_levels, a.score_draws, a.score_scales) == ("score", 7, 3, [1, 2])
    d = p.parse_args(["--mode", "score"])
    assert (d.score_levels, d.score_draws, d.score_scales) == (10, 4, None)
    full = main.parse_args(["--mode", "score"])
    assert full.score_images is None                                             # no picture given: the training pyramid alone
    one = main.parse_args(["--mode", "score", "--input_image", "scratch.png"])
    assert one.score_images == "scratch.png"
    two = main.parse_args(["--mode", "score", "--input_image", "a.png", "b.png", "c.png"])      # (not tied to the sample batch)
    assert list(two.score_images) == ["a.png", "b.png", "c.png"]
    # the flag's own default, typed out, is a picture that was given
    same = main.parse_args(["--mode", "score", "--input_image", p.get_default("input_image")])
    assert same.score_images == "seascape_composite_dragon.png"
    for bad in (["--score_levels", "0"], ["--score_draws", "0"], ["--score_scales", "2", "1"], ["--score_scales", "-1", "1"]):
        with pytest.raises(SystemExit):
            main.parse_args(["--mode", "score"] + bad)
    # every other command line parses as it did
    old = main.parse_args(["--mode", "sample"])
    assert old.input_image == "seascape_composite_dragon.png" and old.mode == "sample"


def test_edit_map_file_is_what_edit_reads(tmp_path):
    """The PNG MultiscaleTrainer.score writes for a picture -- 8-bit gray, value = round(255 * strength) -- read back the way
    `--mode edit --edit_map` reads its file is the strength map to 1/255."""
    from PIL import Image
    e = score_edit_map(torch.linspace(0, 4, 20 * 30).reshape(20, 30), torch.linspace(1, 3, 20 * 30).reshape(20, 30))
    arr = e.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).numpy()
    path = os.path.join(str(tmp_path), "score_edit_map.png")
    Image.fromarray(arr, mode="L").save(path)
    back = torch.from_numpy(np.asarray(Image.open(path).convert("L").resize((30, 20), Image.BILINEAR), dtype=np.float32).copy()).div(255)
    assert tuple(back.shape) == (20, 30) and float(back.min()) >= 0.0 and float(back.max()) <= 1.0
    assert float((back - e).abs().max()) <= 0.5 / 255 + 1e-6
