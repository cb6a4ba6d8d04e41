"""The drivers of `MultiscaleTrainer` through `MultiScaleGaussianDiffusion.sampling(...)`, on the GPU: a driver is
`sample_scales` inside the scope of its options, bit for bit, what the caller configured on `ema_model` stays in force
during the call, and it is there -- the same objects -- afterwards.  The C1 recipe of tests/test_gpu_tile.py (golden pyramid,
closed-form weights, dim 32, T = 20), batch 2, per-sample seeds.  tests/test_sampling_scope_host.py has the scope itself."""
import pytest
import torch

from sinddm_amd.functions import _layout_pyramid, keep_mask_pyramid, layout_blocks
from sinddm_amd.sampler import sampling_defaults
from sinddm_amd.synth import hash_randn
from test_gpu_tile import _trainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KW = dict(batch_size=2, seeds=[11, 77], save_images=False)


def _same(got, want, sizes):
    assert [tuple(g.shape) for g in got] == [(2, 3) + tuple(hw) for hw in sizes] == [tuple(w.shape) for w in want]
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_paint2image_is_sample_scales_inside_the_scope(golden, tmp_path):
    tr, meta = _trainer(golden, tmp_path)
    em, n = tr.ema_model, tr.n_scales
    em.sample_steps = 3                                                  # the caller's: in force during the call, kept after it
    sizes = [tuple(em.target_size(s, (1, 1))) for s in range(n)]
    lay = (hash_randn((2, 3) + sizes[-1], 70) * 0.6).clamp(-1, 1)
    got = tr.paint2image(lay, strength=[0.25, 0.5], **KW)
    tab = sampling_defaults()
    assert em.sample_steps == 3
    assert all(getattr(em, k) == tab[k] for k in ("layout_maps", "layout_down", "layout_strength", "layout_t_min", "layout_gain"))
    pyr, blocks = _layout_pyramid(lay, sizes), layout_blocks(8, tr.scale_factor, n)
    with em.sampling(layout_maps={s: pyr[s].to(DEV).contiguous() for s in range(n)}, layout_down={s: blocks[s] for s in range(n)},
                     layout_strength=0.5, layout_t_min=0, layout_gain=[0.5, 1.0]):
        want = tr.sample_scales(scale_mul=(1, 1), **KW)
    _same(got, want, sizes)
    assert not torch.equal(got[-1], tr.sample_scales(scale_mul=(1, 1), **KW)[-1])      # (the layout did pull)
    em.sample_steps = None
    assert not torch.equal(got[-1], tr.paint2image(lay, strength=[0.25, 0.5], **KW)[-1])   # (and the three steps were in force)


def test_inpaint_is_sample_scales_inside_the_scope_and_hands_back_the_callers_maps(golden, tmp_path):
    tr, meta = _trainer(golden, tmp_path)
    em, n = tr.ema_model, tr.n_scales
    sizes = [tuple(em.image_sizes[s]) for s in range(n)]
    H, W = sizes[-1]
    mine = {0: (torch.zeros(sizes[0], device=DEV), torch.zeros((3,) + sizes[0], device=DEV))}
    em.keep_maps = mine                                                  # the caller's own maps: not the call's, back after it
    mask = torch.ones(H, W)
    mask[H // 4:H // 2, W // 3:2 * W // 3] = 0
    got = tr.inpaint(mask, **KW)
    assert em.keep_maps is mine and em.resample is None and em.keep_window is None
    masks = keep_mask_pyramid(mask, sizes, hard=True)
    maps = {s: (masks[s].to(DEV).contiguous(), tr.data_list[s][0][0].contiguous()) for s in range(n)}
    with em.sampling(keep_maps=maps):
        want = tr.sample_scales(**KW)
    assert em.keep_maps is mine
    _same(got, want, sizes)
    known = maps[n - 1][0] == 1
    assert torch.equal(got[-1][:, :, known], maps[n - 1][1][None].expand_as(got[-1])[:, :, known])     # (the mask was the call's)
