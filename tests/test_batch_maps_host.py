"""Per-sample conditioning maps, host side (no GPU): the batched pyramids, the rank slice of per-sample rows, the strength ->
(max, gain) split, the command line's one-value-per-job flags, the checks of `MultiScaleGaussianDiffusion` and the drivers
on a leading batch dimension, the ABI mirror, and the argument validation of sinddm_sample_chain_batch, which happens
before any device work -- through the library with fake pointers, and in a stand-alone program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from sinddm_amd import _lib
from sinddm_amd import dist as sdist
from sinddm_amd.configs import build_diffusion
from sinddm_amd.functions import _layout_pyramid, keep_mask_pyramid, split_strength

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(12, 17), (25, 34), (50, 67)]


def _rand(shape, key):
    return torch.from_numpy(np.random.RandomState(key).standard_normal(shape).astype(np.float32))


# ---- the pyramids -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hard", [True, False])
def test_batched_mask_pyramid_is_the_unbatched_rows(hard):
    masks = torch.ones(3, 50, 67)
    masks[0, 5:21, 7:30] = 0                                             # edges off the scale ratios
    masks[1, 10:40, 20:60] = 0
    masks[2] = (_rand((50, 67), 1) > -1.0).float()                       # scattered holes: hard masks give most of it up
    pyr = keep_mask_pyramid(masks, SIZES, hard=hard, batch=True)
    assert [tuple(t.shape) for t in pyr] == [(3,) + hw for hw in SIZES] and all(t.dtype == torch.float32 for t in pyr)
    for b in range(3):
        for t, one in zip(pyr, keep_mask_pyramid(masks[b], SIZES, hard=hard)):
            assert torch.equal(t[b], one)
    assert not torch.equal(pyr[0][0], pyr[0][1])
    for bad in (masks[0], masks[None]):
        with pytest.raises(ValueError):
            keep_mask_pyramid(bad, SIZES, batch=True)


def test_batched_layout_pyramid_is_the_unbatched_rows():
    lay = _rand((4, 3, 50, 67), 2).clamp(-1, 1)
    pyr = _layout_pyramid(lay, SIZES)
    assert [tuple(t.shape) for t in pyr] == [(4, 3) + hw for hw in SIZES]
    for b in range(4):
        for t, one in zip(pyr, _layout_pyramid(lay[b], SIZES)):
            assert torch.equal(t[b], one)
    assert torch.equal(pyr[-1], lay)
    with pytest.raises(ValueError):
        _layout_pyramid(lay[:, :2], SIZES)


# ---- the rank slice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,world", [(3, 1), (4, 2), (5, 2), (7, 3), (4, 3), (16, 3)])
def test_shard_rows_cut_where_shard_seeds_cuts(B, world, monkeypatch):
    rows, seeds = _rand((B, 2, 3), 3), [1000 + 3 * b for b in range(B)]
    boxes = [[[b, b, 1, 1]] for b in range(B)]
    monkeypatch.setattr(sdist, "world_size", lambda: world)
    parts, lists = [], []
    for r in range(world):
        monkeypatch.setattr(sdist, "rank", lambda r=r: r)
        part, mine = sdist.shard_rows(rows), sdist.shard_seeds(seeds)
        assert part.shape[0] == len(mine) == sdist.local_batch(B)
        o = sdist.shard_offset(B)
        assert torch.equal(part, rows[o:o + len(mine)]) and mine == seeds[o:o + len(mine)]
        parts.append(part)
        lists += sdist.shard_rows(boxes)
    assert torch.equal(torch.cat(parts), rows) and lists == boxes        # the gathered batch is the single process's


def test_sample_scales_takes_this_ranks_rows(monkeypatch):
    from sinddm_amd.trainer import MultiscaleTrainer
    net, d = build_diffusion("C1", dim=16, device="cpu")
    tr = MultiscaleTrainer.__new__(MultiscaleTrainer)
    tr.ema_model = d
    H, W = d.image_sizes[0]
    B = 5
    m, k0, lay = _rand((B, H, W), 4), _rand((B, 3, H, W), 5), _rand((B, 3, H, W), 6)
    shared = _rand((3, H, W), 7)
    d.keep_maps = {0: (m, shared), 1: (_rand((9, 9), 8), _rand((3, 9, 9), 9))}
    d.layout_maps, d.layout_gain = {0: lay}, [0.1 * b for b in range(B)]
    d.roi_bbs_batch = [[[b, 0, 1, 1]] for b in range(B)]
    monkeypatch.setattr(sdist, "world_size", lambda: 2)
    monkeypatch.setattr(sdist, "rank", lambda: 1)
    got = tr._local_batch_maps(B)
    assert torch.equal(got["keep_maps"][0][0], m[3:]) and got["keep_maps"][0][1] is shared       # ranks: 3 + 2
    assert got["keep_maps"][1][0] is d.keep_maps[1][0]
    assert torch.equal(got["layout_maps"][0], lay[3:]) and got["layout_gain"] == [0.1 * 3, 0.1 * 4]
    assert got["roi_bbs_batch"] == [[[3, 0, 1, 1]], [[4, 0, 1, 1]]] and "roi_target_patch_batch" not in got
    with pytest.raises(ValueError, match="rows for batch_size=6"):
        tr._local_batch_maps(B + 1)
    d.keep_maps, d.layout_maps, d.layout_gain, d.roi_bbs_batch = {0: (m[0], k0[0])}, {0: lay[0]}, None, None
    assert tr._local_batch_maps(B) == {}                                 # nothing per sample: nothing is touched


# ---- strength -> (max, gain) -----------------------------------------------------------------------------------------------
def test_split_strength():
    assert split_strength(0.5, 4) == (0.5, None) and split_strength(1, 2) == (1.0, None)
    top, gain = split_strength([0.25, 1.0, 0.5, 0.0], 4)
    assert top == 1.0 and gain == [0.25, 1.0, 0.5, 0.0]
    top, gain = split_strength(torch.tensor([0.3, 0.6, 0.15]), 3)
    assert top == float(np.float32(0.6)) and gain[1] == 1.0
    for v, g_b in zip((0.3, 0.6, 0.15), gain):                           # the step's fp32 product is the value to one rounding
        assert abs(float(np.float32(top) * np.float32(g_b)) - float(np.float32(v))) <= 2.0 ** -24 * v
        assert 0.0 <= g_b <= 1.0
    assert split_strength([0.0, 0.0], 2) == (0.0, [1.0, 1.0])
    for bad, B in (([0.5, 0.5], 3), ([0.5, 1.5], 2), ([-0.1, 0.5], 2)):
        with pytest.raises(ValueError):
            split_strength(bad, B)


# ---- the command line -----------------------------------------------------------------------------------------------------
def test_cli_one_value_per_job(capsys):
    sys.path.insert(0, REPO)
    try:
        import main as cli
    finally:
        sys.path.remove(REPO)
    a = cli.parse_args(["--mode", "inpaint", "--sample_batch_size", "6", "--mask_path", "a.png", "b.png", "c.png"])
    assert isinstance(a.mask_path, cli.Jobs) and a.mask_path == ["a.png", "b.png", "c.png"]
    assert cli.job_values(a.mask_path, 6) == ["a.png", "b.png", "c.png", "a.png", "b.png", "c.png"]      # sample b: value b % N
    a = cli.parse_args(["--mode", "outpaint", "--sample_batch_size", "4", "--anchor", "0", "1", "0.5", "0"])
    assert a.anchor == [[0.0, 1.0], [0.5, 0.0]] and cli.job_values(a.anchor, 4) == [[0.0, 1.0], [0.5, 0.0]] * 2
    a = cli.parse_args(["--mode", "paint2image", "--sample_batch_size", "4", "--input_image", "p.png", "q.png",
                        "--layout_strength", "0.25", "0.5", "0.75", "1"])
    assert a.input_image == ["p.png", "q.png"] and cli.job_values(a.layout_strength, 4) == [0.25, 0.5, 0.75, 1.0]
    # one value is today's command line: scalars, not lists, and the same namespace
    a = cli.parse_args(["--mask_path", "a.png", "--input_image", "p.png", "--layout_strength", "0.5", "--anchor", "0", "1"])
    assert (a.mask_path, a.input_image, a.layout_strength, a.anchor) == ("a.png", "p.png", 0.5, [0.0, 1.0])
    assert not any(isinstance(v, cli.Jobs) for v in vars(a).values()) and cli.job_values(a.anchor, 4) == [0.0, 1.0]
    d = cli.parse_args([])
    assert (d.mask_path, d.layout_strength, d.anchor) == (None, 1.0, [0.5, 0.5]) and isinstance(d.input_image, str)
    for argv in (["--sample_batch_size", "4", "--mask_path", "a", "b", "c"],                     # 4 % 3 != 0
                 ["--sample_batch_size", "3", "--anchor", "0", "1", "1", "0"],
                 ["--sample_batch_size", "5", "--input_image", "p", "q"],
                 ["--sample_batch_size", "3", "--layout_strength", "0.5", "1"],
                 ["--sample_batch_size", "4", "--layout_strength", "0.5", "1.5"],                # a value out of range
                 ["--anchor", "0", "1", "0.5"]):                                                 # half a pair
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    assert "multiple of 3" in capsys.readouterr().err


# ---- the diffusion's checks -------------------------------------------------------------------------------------------------
def test_entries_accept_the_running_batch_and_nothing_else():
    net, d = build_diffusion("C1", dim=16, device="cpu")
    H, W = d.image_sizes[0]
    x = torch.zeros(4, 3, H, W)
    assert d.layout_gain is None and d.roi_bbs_batch is None and d.roi_target_patch_batch is None
    for m, k0 in ((torch.zeros(4, H, W), torch.zeros(3, H, W)), (torch.zeros(H, W), torch.zeros(4, 3, H, W)),
                  (torch.zeros(4, H, W), torch.zeros(4, 3, H, W))):
        d.keep_maps = {0: (m, k0)}
        got = d._keep_entry(0, x)
        assert got[0].shape == m.shape and got[1].shape == k0.shape
    for m, k0 in ((torch.zeros(3, H, W), torch.zeros(3, H, W)), (torch.zeros(H, W), torch.zeros(5, 3, H, W)),
                  (torch.zeros(1, H, W), torch.zeros(3, H, W)), (torch.zeros(4, H, W + 1), torch.zeros(3, H, W))):
        d.keep_maps = {0: (m, k0)}
        with pytest.raises(_lib.SinddmError, match=r"keep_maps\[0\].*expected"):
            d._keep_entry(0, x)
    d.keep_maps = None
    d.layout_down = {0: 4}
    d.layout_maps = {0: torch.zeros(4, 3, H, W)}
    assert d._layout_entry(0, x)[0].shape == (4, 3, H, W)
    for lay in (torch.zeros(2, 3, H, W), torch.zeros(4, 1, H, W), torch.zeros(4, 3, H, W, dtype=torch.float64)):
        d.layout_maps = {0: lay}
        with pytest.raises(_lib.SinddmError, match=r"layout_maps\[0\].*expected"):
            d._layout_entry(0, x)
    assert d._layout_gain_for(4, "cpu") is None
    d.layout_gain = [0.0, 0.25, 1.0, 0.5]
    assert d._layout_gain_for(4, "cpu").tolist() == [0.0, 0.25, 1.0, 0.5] and d._layout_gain_for(4, "cpu").dtype == torch.float32
    d.layout_gain = torch.tensor([0.0, 0.25, 1.0, 0.5], dtype=torch.float64)
    assert d._layout_gain_for(4, "cpu").tolist() == [0.0, 0.25, 1.0, 0.5]
    with pytest.raises(ValueError, match="layout_gain has 4 values, the batch 3"):
        d._layout_gain_for(3, "cpu")
    for bad in ([0.0, 0.25, 1.5, 0.5], [0.0, -0.25, 1.0, 0.5], [0.0, float("nan"), 1.0, 0.5]):
        d.layout_gain = bad
        with pytest.raises(ValueError, match="outside"):
            d._layout_gain_for(4, "cpu")


def test_per_sample_roi_maps_are_the_shared_rows():
    net, d = build_diffusion("C1", dim=16, device="cpu")
    H, W = d.image_sizes[0]
    patch = lambda k: [_rand((1, 3, 5, 4), k + s).clamp(-1, 1) for s in range(d.n_scales)]
    lists = [[[8, 10, 20, 16]], [[8, 10, 20, 16], [30, 40, 24, 20]], []]
    d.roi_target_patch = patch(10)
    shared = []
    for bbs in lists:
        d.roi_bbs, d._roi_cache = bbs, {}
        shared.append(tuple(t.clone() for t in d.roi_edit_maps(0, H, W, "cpu")))
    d.roi_bbs, d.roi_bbs_batch, d._roi_cache = [], lists, {}
    ew, ec = d.roi_edit_maps(0, H, W, "cpu")
    assert tuple(ew.shape) == (3, H, W) and tuple(ec.shape) == (3, 3, H, W)
    for b in range(3):
        assert torch.equal(ew[b], shared[b][0]) and torch.equal(ec[b], shared[b][1])
    assert bool((ew[2] == 1).all()) and not torch.equal(ew[0], ew[1])
    assert d.roi_edit_maps(0, H, W, "cpu")[0] is ew                      # cached
    d.roi_target_patch_batch = [patch(10), patch(20), patch(30)]         # per-sample patches: row 0 has the shared one's
    ew2, ec2 = d.roi_edit_maps(0, H, W, "cpu")
    assert torch.equal(ew2, ew) and torch.equal(ec2[0], ec[0]) and not torch.equal(ec2[1], ec[1])
    x = _rand((3, 3, H, W), 40)
    want = ew2[:, None] * x + ec2
    assert torch.equal(d.roi_patch_modification(x.clone(), scale=0), want)
    d.roi_target_patch_batch = [patch(10)]
    with pytest.raises(ValueError, match="roi_target_patch_batch"):
        d.roi_edit_maps(0, H, W, "cpu")


def test_drivers_build_per_sample_maps_and_clear_them():
    from sinddm_amd.trainer import MultiscaleTrainer
    net, d = build_diffusion("C1", dim=16, device="cpu")
    tr = MultiscaleTrainer.__new__(MultiscaleTrainer)                    # (the drivers alone: no data folder, no optimiser)
    tr.ema_model, tr.n_scales, tr.scale_factor, tr.device = d, d.n_scales, d.scale_factor, "cpu"
    tr.data_list = [[[_rand((3,) + tuple(d.image_sizes[s]), 50 + s).clamp(-1, 1)]] for s in range(d.n_scales)]
    seen = {}

    def sample_scales(**kw):
        seen.update(keep=d.keep_maps, lay=d.layout_maps, g=d.layout_strength, gain=d.layout_gain, boxes=d.roi_bbs_batch,
                    shared_boxes=d.roi_bbs, kw=kw)
        raise RuntimeError("stop here")

    tr.sample_scales = sample_scales
    H, W = d.image_sizes[d.n_scales - 1]
    masks = torch.ones(2, H, W)
    masks[1, 3:9, 4:11] = 0
    with pytest.raises(RuntimeError, match="stop here"):
        tr.inpaint(masks, batch_size=2, save_images=False)
    assert d.keep_maps is None
    for s in range(d.n_scales):
        m, k0 = seen["keep"][s]
        assert tuple(m.shape) == (2,) + tuple(d.image_sizes[s]) and tuple(k0.shape) == (3,) + tuple(d.image_sizes[s])
        assert bool((m[0] == 1).all()) and not bool((m[1] == 1).all())
    for bad in (torch.ones(3, H, W), torch.ones(2, H, W - 1)):
        with pytest.raises(ValueError, match="inpaint"):
            tr.inpaint(bad, batch_size=2, save_images=False)
    with pytest.raises(RuntimeError, match="stop here"):
        tr.outpaint((1, 1.5), anchor=[(0.5, 0.0), (0.5, 1.0)], batch_size=2, save_images=False)
    m, k0 = seen["keep"][d.n_scales - 1]
    Wc = int(W * 1.5)
    assert tuple(m.shape) == (2, H, Wc) and tuple(k0.shape) == (2, 3, H, Wc)
    assert bool((m[0][:, :W] == 1).all()) and bool((m[0][:, W:] == 0).all()) and bool((m[1][:, Wc - W:] == 1).all())
    assert torch.equal(k0[0][:, :, :W], tr.data_list[-1][0][0]) and torch.equal(k0[1][:, :, Wc - W:], tr.data_list[-1][0][0])
    with pytest.raises(ValueError, match="anchors"):
        tr.outpaint((1, 1.5), anchor=[(0.5, 0.0)] * 3, batch_size=2, save_images=False)
    with pytest.raises(RuntimeError, match="stop here"):                 # one pair: the shared maps, as ever
        tr.outpaint((1, 1.5), anchor=(0.5, 1.0), batch_size=2, save_images=False)
    assert seen["keep"][0][0].dim() == 2 and seen["keep"][0][1].dim() == 3
    lay = _rand((2, 3, H, W), 60).clamp(-1, 1)
    with pytest.raises(RuntimeError, match="stop here"):
        tr.paint2image(lay, batch_size=2, strength=[0.25, 0.5], save_images=False)
    assert seen["g"] == 0.5 and seen["gain"] == [0.5, 1.0]
    assert all(tuple(seen["lay"][s].shape) == (2, 3) + tuple(d.target_size(s, (1, 1))) for s in range(d.n_scales))
    assert torch.equal(seen["lay"][d.n_scales - 1], lay)
    assert d.layout_maps is None and d.layout_gain is None and d.layout_strength == 1.0
    for kw in (dict(layout=lay, batch_size=3), dict(layout=lay, batch_size=2, strength=[0.5]),
               dict(layout=lay, batch_size=2, strength=[0.5, 1.5])):
        with pytest.raises(ValueError):
            tr.paint2image(save_images=False, **kw)
        assert d.layout_maps is None and d.layout_gain is None
    # roi: B box lists
    with pytest.raises(RuntimeError, match="stop here"):
        tr.roi_guided_sampling(target_roi=[2, 2, 8, 8], roi_bb_list=[[[1, 1, 4, 4]], [[5, 5, 4, 4], [9, 9, 4, 4]]], batch_size=2,
                               per_sample=True, save_images=False)
    assert seen["boxes"] == [[[1, 1, 4, 4]], [[5, 5, 4, 4], [9, 9, 4, 4]]] and seen["shared_boxes"] == []
    assert d.roi_bbs_batch is None and d.roi_guided_sampling is False
    with pytest.raises(ValueError, match="box lists"):
        tr.roi_guided_sampling(target_roi=[2, 2, 8, 8], roi_bb_list=[[[1, 1, 4, 4]]], batch_size=2, per_sample=True)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_batch_entry_declared_bound_and_mirrored():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    lib = _lib.load()
    assert re.search(r"\bint\s+sinddm_sample_chain_batch\s*\(", txt) and "sinddm_sample_chain_batch" in _lib.ABI_SYMBOLS
    assert hasattr(lib, "sinddm_sample_chain_batch")
    m = re.search(r"typedef struct sinddm_batch_opts \{(.*?)\} sinddm_batch_opts;", txt, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"^\s*[\w ]+?\*?\s*(\w+);", body, re.M) == [f[0] for f in _lib.BatchOpts._fields_] == \
        ["edit_per_sample", "keep_mask_per_sample", "keep_x0_per_sample", "layout_per_sample", "layout_gain"]
    assert C.sizeof(_lib.BatchOpts) == 4 * C.sizeof(C.c_int) + C.sizeof(C.c_void_p)
    lo, bo = lib.sinddm_sample_chain_layout.argtypes, lib.sinddm_sample_chain_batch.argtypes
    assert list(bo[:-1]) == list(lo) and bo[-1] is C.POINTER(_lib.BatchOpts)
    assert int(re.search(r"#define SINDDM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 3        # additive
    assert not _lib.missing_symbols()


def test_batch_entry_validates_without_a_device():
    """Fake non-null device pointers and an empty workspace: a call that passes the checks fails next on the workspace
    (-3), a misuse returns SINDDM_E_BADARG (-1); nothing is enqueued or dereferenced either way."""
    lib = _lib.load()
    n = 2
    coefs = (_lib.StepCoefs * n)()
    tl = (C.c_int * n)(1, 0)
    flag = C.c_int(7)
    g = (C.c_float * n)(1.0, 0.5)
    ab = (C.c_float * (2 * n))(1.0, 0.0, 1.0, 0.0)
    P = 4096                                                             # (16-byte aligned)

    def chain(flags=(0, 0, 0, 0), gain=None, edit=False, keep=False, lay=False, H=8, W=8, mask_ptr=P, null_bo=False):
        opts = _lib.ChainOpts(P if edit else None, P if edit else None, None)
        kopts = _lib.KeepOpts(mask_ptr, P, C.cast(ab, C.POINTER(C.c_float))) if keep else None
        lopts = _lib.LayoutOpts(P, 4, C.cast(g, C.POINTER(C.c_float)), P) if lay else None
        bo = _lib.BatchOpts(*flags, gain)
        return lib.sinddm_sample_chain_batch(P, P, P, P, P, None, coefs, tl, n, 0.0, 1, 0, 160, 4, H, W, P, 0, None, None,
                                             C.byref(flag), C.byref(opts), 0, 0, C.byref(kopts) if keep else None, None, None,
                                             C.byref(lopts) if lay else None, None if null_bo else C.byref(bo))

    OK, BAD = -3, -1
    assert chain(null_bo=True) == OK and chain() == OK
    assert chain((1, 1, 1, 1), gain=P, edit=True, keep=True, lay=True) == OK
    assert chain((0, 1, 0, 0), keep=True) == OK and chain((0, 0, 1, 0), keep=True) == OK
    assert chain(gain=P + 4, lay=True) == OK
    # a flag set whose pointer is NULL
    assert chain((1, 0, 0, 0)) == BAD and chain((1, 0, 0, 0), keep=True, lay=True) == BAD
    assert chain((0, 1, 0, 0)) == BAD and chain((0, 0, 1, 0), edit=True) == BAD
    assert chain((0, 0, 0, 1)) == BAD and chain((0, 0, 0, 1), edit=True, keep=True) == BAD
    # layout_gain without a layout; not 4-byte aligned
    assert chain(gain=P) == BAD and chain(gain=P, keep=True) == BAD
    assert chain(gain=P + 2, lay=True) == BAD and chain(gain=P + 1, lay=True) == BAD
    # the 16-byte rule: a per-sample map off the boundary is refused like a shared one
    assert chain((0, 1, 0, 0), keep=True, mask_ptr=P + 4) == BAD
    # 9x9: H*W % 4 != 0, not the plain fused route -- per-sample slices of 81 floats are fine there
    assert chain((1, 1, 1, 1), gain=P, edit=True, keep=True, lay=True, H=9, W=9) == OK
    assert flag.value == 7


SAN_MAIN = r"""
#include <cstdio>
#include <vector>
#include "batch_check.h"
using namespace sinddm;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
int main() {
    std::vector<float> buf(16 * 3 * 9 * 9 + 8);                 // stands for a device map: B = 16 slices of 3 x 9 x 9
    const float* P = buf.data();
    alignas(4) float gains[16] = {};
    BatchStrides s;
    CHECK(batch_strides(nullptr, P, P, P, P, P, 9, 9, false, &s) == 0 && s.sew == 0 && s.sl == 0);
    sinddm_batch_opts bo{};
    CHECK(batch_strides(&bo, nullptr, nullptr, nullptr, nullptr, nullptr, 9, 9, true, &s) == 0 && s.skm == 0);
    bo = sinddm_batch_opts{1, 1, 1, 1, gains};
    CHECK(batch_strides(&bo, P, P, P, P, P, 9, 9, false, &s) == 0);
    CHECK(s.sew == 81 && s.sec == 243 && s.skm == 81 && s.skx == 243 && s.sl == 243);
    CHECK(batch_strides(&bo, P, P, P, P, P, 9, 9, true, &s) == SINDDM_E_BADARG && s.sew == 0);     // 81 % 4 != 0 under f32x4 loads
    CHECK(batch_strides(&bo, P, P, P, P, P, 8, 10, true, &s) == 0 && s.skm == 80 && s.skx == 240);
    for (int f = 0; f < 4; ++f) {                                // a flag set whose pointer is NULL
        sinddm_batch_opts one{f == 0, f == 1, f == 2, f == 3, nullptr};
        CHECK(batch_strides(&one, f == 0 ? nullptr : P, f == 0 ? nullptr : P, f == 1 ? nullptr : P, f == 2 ? nullptr : P,
                            f == 3 ? nullptr : P, 8, 8, true, &s) == SINDDM_E_BADARG);
        CHECK(batch_strides(&one, P, P, P, P, P, 8, 8, true, &s) == 0);
    }
    sinddm_batch_opts half{1, 0, 0, 0, nullptr};
    CHECK(batch_strides(&half, P, nullptr, P, P, P, 8, 8, true, &s) == SINDDM_E_BADARG);          // the pair goes together
    sinddm_batch_opts gn{0, 0, 0, 0, gains};
    CHECK(batch_strides(&gn, P, P, P, P, nullptr, 8, 8, true, &s) == SINDDM_E_BADARG);            // gain without a layout
    CHECK(batch_strides(&gn, P, P, P, P, P, 8, 8, true, &s) == 0 && s.sl == 0);
    gn.layout_gain = reinterpret_cast<const float*>(reinterpret_cast<const char*>(gains) + 2);
    CHECK(batch_strides(&gn, P, P, P, P, P, 8, 8, true, &s) == SINDDM_E_BADARG);                  // not 4-byte aligned
    sinddm_batch_opts big{0, 0, 1, 0, nullptr};
    CHECK(batch_strides(&big, P, P, P, P, P, 40000, 40000, false, &s) == SINDDM_E_BADSHAPE);      // 3 H W past an int
    CHECK(batch_strides(&big, P, P, P, P, P, 26754, 26754, false, &s) == 0 && s.skx == 3 * 26754 * 26754);
    // the second half-batch's slices: b0 = 8 of 16, every slice inside the buffer; NULL stays NULL; shared maps do not move
    bo = sinddm_batch_opts{1, 1, 1, 1, gains};
    CHECK(batch_strides(&bo, P, P, P, P, P, 9, 9, false, &s) == 0);
    CHECK(batch_slice(P, 8, s.skm) == P + 8 * 81 && batch_slice(P, 8, s.skx) == P + 8 * 243 && batch_slice(P, 15, s.sl)[242] == 0.0f);
    CHECK(batch_slice(nullptr, 8, s.skx) == nullptr && batch_slice(P, 8, 0) == P && batch_slice(P, 0, s.sec) == P);
    CHECK(batch_slice(P, 65535, 0x7fffffff) == P + (size_t)65535 * 0x7fffffffu);                  // 64-bit offset, no int overflow
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails != 0;
}
"""


def _host_cxx():
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.mark.skipif(_host_cxx() is None, reason="no host C++ compiler")
def test_pre_device_checks_under_sanitizers(tmp_path):
    """sinddm_amd/csrc/batch_check.h is all of sinddm_sample_chain_batch that runs before device work, and it is free of HIP:
    a stand-alone program with its own main calls it under -fsanitize=address,undefined."""
    src, exe = tmp_path / "batch_check_main.cpp", tmp_path / "batch_check_main"
    src.write_text(SAN_MAIN)
    subprocess.check_call([_host_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "sinddm_amd", "csrc"), str(src), "-o",
                           str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
