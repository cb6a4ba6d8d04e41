"""The sampling options, host side (no GPU, no library): `sampler.sampling_defaults` is the one list of what a run reads off
the diffusion object, `MultiScaleGaussianDiffusion.sampling(**options)` sets some of them for a `with` block and puts back the
very objects it found, and every driver of `MultiscaleTrainer` goes through it: after a call, returned or raised, the model
is as the caller configured it -- not at the defaults."""
from pathlib import Path

import numpy as np
import pytest
import torch

from sinddm_amd.configs import build_diffusion
from sinddm_amd.sampler import sampling_defaults
from sinddm_amd.trainer import MultiscaleTrainer

NAMES = ["tile", "keep_maps", "keep_gated", "keep_window", "sample_seeds", "seed_mix", "resample", "layout_maps", "layout_down",
         "layout_strength", "layout_t_min", "layout_gain", "roi_bbs_batch", "roi_target_patch_batch", "sample_steps",
         "sample_spacing", "solver_order", "eta", "noise_fn", "draw_log", "two_streams", "chain_noise", "chain_guided",
         "roi_guided_sampling", "clip_guided_sampling"]


def _rand(shape, key):
    return torch.from_numpy(np.random.RandomState(key).standard_normal(shape).astype(np.float32))


def _state(d):
    return {k: getattr(d, k) for k in NAMES}


def _same_objects(d, state):
    return [k for k in NAMES if getattr(d, k) is not state[k]] == []


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_a_fresh_model_carries_the_table():
    tab = sampling_defaults()
    assert sorted(tab) == sorted(NAMES) and len(NAMES) == 25
    _, d = build_diffusion("C1", dim=16, device="cpu")
    _, d2 = build_diffusion("C1", dim=16, device="cpu")
    for k, v in tab.items():
        assert k in vars(d) and type(getattr(d, k)) is type(v) and getattr(d, k) == v, k      # (plain attributes)
    assert (tab["tile"], tab["layout_down"], tab["layout_strength"], tab["two_streams"], tab["eta"]) == ((False, False), {}, 1.0, True, 1.0)
    assert d.layout_down is not d2.layout_down and sampling_defaults()["layout_down"] is not tab["layout_down"]
    for k in ("omega", "train_tile", "train_weights", "train_crop", "crop_fn", "roi_bbs", "roi_target_patch", "clip_model"):
        assert k not in tab and hasattr(d, k)


# ---- the scope ----------------------------------------------------------------------------------------------------------------
def test_scope_restores_by_identity_nests_and_refuses_unknown_names():
    _, d = build_diffusion("C1", dim=16, device="cpu")
    d.keep_maps, d.layout_down, d.sample_seeds = {0: "mine"}, {1: 4}, [1, 2]
    before = _state(d)
    inner_maps, seeds = {0: "theirs"}, [3, 4]
    with d.sampling(keep_maps=inner_maps, tile=(True, True)) as got:
        assert got is d and d.keep_maps is inner_maps and d.tile == (True, True) and d.sample_seeds is before["sample_seeds"]
        with d.sampling(keep_maps=None, sample_seeds=seeds):
            assert d.keep_maps is None and d.sample_seeds is seeds and d.tile == (True, True)
        assert d.keep_maps is inner_maps and d.sample_seeds is before["sample_seeds"]
    assert _same_objects(d, before)
    with pytest.raises(RuntimeError, match="inside"):
        with d.sampling(layout_down={}, eta=0.0, roi_guided_sampling=True):
            assert d.eta == 0.0 and d.roi_guided_sampling is True
            raise RuntimeError("inside")
    assert _same_objects(d, before)
    with d.sampling():                                                   # (nothing named: nothing touched)
        pass
    # an unknown name: TypeError, and not even the known names beside it are set
    for bad in (dict(keep_map=None), dict(tile=(True, True), omega=0.3), dict(train_tile=(True, True)), dict(roi_bbs=[])):
        with pytest.raises(TypeError, match="not a sampling option"):
            with d.sampling(**bad):
                raise AssertionError("the block must not run")
        assert _same_objects(d, before)
    # no value is looked at: the readers validate when a run starts
    with d.sampling(resample="nonsense", keep_window=-3, sample_steps=object()):
        assert d.resample == "nonsense"
        with pytest.raises(ValueError):
            d._resample_cfg()
    assert _same_objects(d, before)


# ---- the drivers --------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path):
    _, d = build_diffusion("C1", dim=16, device="cpu")
    tr = MultiscaleTrainer.__new__(MultiscaleTrainer)                    # (the drivers alone: no data folder, no optimiser)
    tr.ema_model, tr.n_scales, tr.scale_factor, tr.device = d, d.n_scales, d.scale_factor, "cpu"
    tr.results_folder = Path(str(tmp_path))
    tr.data_list = [[[_rand((3,) + tuple(d.image_sizes[s]), 50 + s).clamp(-1, 1)]] for s in range(d.n_scales)]
    H, W = d.image_sizes[0]
    # what a caller configured: the drivers must hand it back
    d.keep_maps = {0: (torch.ones(H, W), torch.zeros(3, H, W))}
    d.tile, d.sample_steps, d.layout_strength = (True, False), 3, 0.5
    return tr, d


def _driver_calls(tr, d):
    """(name, call, what the stub must see inside)"""
    H, W = d.image_sizes[d.n_scales - 1]
    mask = torch.ones(H, W)
    mask[3:9, 4:11] = 0
    ramp = torch.linspace(0, 1, W).expand(H, W).contiguous()
    lay = _rand((2, 3, H, W), 60).clamp(-1, 1)
    kw = dict(batch_size=2, save_images=False)
    pre = d.keep_maps
    kept = lambda gated, rs, win: (lambda: d.keep_maps is not pre and sorted(d.keep_maps) == list(range(d.n_scales))
                                   and d.keep_gated is gated and d.resample == rs and d.keep_window == win)
    return [
        ("inpaint", lambda: tr.inpaint(mask, resample=2, jump_length=3, window=16, **kw), kept(False, (2, 3), 16)),
        ("outpaint", lambda: tr.outpaint((1, 1.5), **kw), kept(False, None, None)),
        ("edit", lambda: tr.edit(ramp, **kw), kept(True, None, None)),
        ("paint2image", lambda: tr.paint2image(lay, strength=[0.375, 0.75], t_min=2, down=4, **kw),
         lambda: (d.layout_strength, d.layout_t_min, d.layout_gain) == (0.75, 2, [0.5, 1.0])
         and sorted(d.layout_maps) == sorted(d.layout_down) == list(range(d.n_scales)) and d.keep_maps is pre),
        ("roi_guided_sampling", lambda: tr.roi_guided_sampling(target_roi=[2, 2, 8, 8], per_sample=True,
                                                               roi_bb_list=[[[1, 1, 4, 4]], [[5, 5, 4, 4]]], **kw),
         lambda: d.roi_guided_sampling is True and d.roi_bbs_batch == [[[1, 1, 4, 4]], [[5, 5, 4, 4]]] and d.roi_bbs == []
         and len(d.roi_target_patch) == d.n_scales and d.keep_maps is pre),
    ]


@pytest.mark.parametrize("raising", [False, True], ids=["returns", "raises"])
def test_drivers_leave_the_model_as_they_found_it(tmp_path, raising):
    tr, d = _trainer(tmp_path)
    before, seen = _state(d), []

    def sample_scales(**kw):
        seen.append((check(), d.tile, d.sample_steps))
        if raising:
            raise RuntimeError("stop here")
        return ["done"]

    tr.sample_scales = sample_scales
    for name, call, check in _driver_calls(tr, d):
        if raising:
            with pytest.raises(RuntimeError, match="stop here"):
                call()
        else:
            assert call() == ["done"], name
        assert seen.pop() == (True, (True, False), 3), name               # the driver's values, beside the caller's
        assert _same_objects(d, before), name
    # ROI guidance leaves its boxes and patches behind, as the reference does; the switch is off again
    assert len(d.roi_target_patch) == d.n_scales and d.roi_guided_sampling is False and d.roi_bbs_batch is None


@pytest.mark.parametrize("raising", [False, True], ids=["returns", "raises"])
def test_sample_scales_with_seeds_leaves_the_model_as_it_found_it(tmp_path, raising):
    tr, d = _trainer(tmp_path)
    d.seed_mix = None
    before, seen = _state(d), []

    def sample(batch_size, scale_0_size=None, s=0):
        seen.append((d.sample_seeds, d.keep_maps, d.tile))
        return torch.zeros((batch_size, 3) + tuple(d.image_sizes[s]))

    def sample_via_scale(batch_size, img, s, **kw):
        seen.append((d.sample_seeds, d.keep_maps, d.tile))
        if raising:
            raise RuntimeError("stop here")
        return torch.zeros((batch_size, 3) + tuple(d.image_sizes[s]))

    d.sample, d.sample_via_scale = sample, sample_via_scale
    if raising:
        with pytest.raises(RuntimeError, match="stop here"):
            tr.sample_scales(batch_size=2, seeds=[11, 77], save_images=False)
    else:
        outs = tr.sample_scales(batch_size=2, seeds=[11, 77], save_images=False)
        assert [tuple(o.shape) for o in outs] == [(2, 3) + tuple(hw) for hw in d.image_sizes]
    assert len(seen) == (2 if raising else d.n_scales)
    assert all(s == ([11, 77], before["keep_maps"], (True, False)) and s[1] is before["keep_maps"] for s in seen)
    assert _same_objects(d, before) and d.sample_seeds is None
    # seeds=None leaves a configured `sample_seeds` in force
    d.sample_seeds = mine = [5, 6]
    del seen[:]
    try:
        tr.sample_scales(batch_size=2, save_images=False)
    except RuntimeError:
        assert raising
    assert seen and all(s[0] is mine for s in seen) and d.sample_seeds is mine


def test_clip_sampling_switches_guidance_on_for_the_call_and_leaves_its_state(tmp_path):
    tr, d = _trainer(tmp_path)
    before, seen = _state(d), []

    class Clip:
        cfg = {"n_aug": 2}

        def get_text_embedding(self, text, template):
            if text == "bad":
                raise KeyError(template)
            return f"{template}:{text}"

    def sample_scales(**kw):
        seen.append((d.clip_guided_sampling, d.text_embedds_hr, d.text_embedds_lr, d.clip_model, kw["batch_size"], kw["desc"]))
        raise RuntimeError("stop here")

    tr.sample_scales, clip = sample_scales, Clip()
    with pytest.raises(KeyError):                                        # the embedding fails: nothing is set
        tr.clip_sampling(clip, "bad", 0.3, 2)
    assert d.clip_model is None and d.clip_strength is None and not seen and _same_objects(d, before)
    with pytest.raises(RuntimeError, match="stop here"):
        tr.clip_sampling(clip, "a prompt", 0.3, 2, quantile=0.7, llambda=0.1)
    on, hr, lr, model, batch, desc = seen.pop()
    assert (on, hr, lr, batch) == (True, "hr:a prompt", "lr:a prompt", 2) and model is clip
    assert desc.startswith("clip_a_prompt_n_aug2_str_0.3_gsi_" + "_".join(str(s) for s in reversed(range(d.n_scales))))
    assert _same_objects(d, before) and d.clip_guided_sampling is False
    # the reference leaves its CLIP state on the model
    assert (d.clip_model, d.clip_strength, d.clip_text, d.quantile, d.llambda) == (clip, 0.3, "a prompt", 0.7, 0.1)
    assert d.guidance_sub_iters == [*reversed(range(d.n_scales))] and d.clip_score == []


def test_a_failed_preparation_sets_nothing(tmp_path):
    tr, d = _trainer(tmp_path)
    before = _state(d)
    tr.sample_scales = lambda **kw: pytest.fail("the run must not start")
    with pytest.raises(ValueError):                                      # extract_patch cannot unpack three numbers
        tr.roi_guided_sampling(target_roi=[2, 2, 8], roi_bb_list=[[1, 1, 4, 4]], batch_size=2, save_images=False)
    assert d.roi_guided_sampling is False and d.roi_bbs == [] and d.roi_target_patch == [] and d.roi_bbs_batch is None
    H, W = d.image_sizes[d.n_scales - 1]
    d.layout_maps = None
    with pytest.raises(ValueError, match="paint2image"):
        tr.paint2image(torch.zeros(3, H, W - 1), batch_size=2, save_images=False)
    assert d.layout_maps is None and d.layout_gain is None and d.layout_down == {}
    assert _same_objects(d, before)
