"""GPU: sinddm_patch_nnf (csrc/patch_nnf.h) and its drivers against float64 brute force (tests/nnf_util.py).

  1. the field of an image against itself is the identity, distance exactly 0: every query, every reference index, the last
     partial tiles, the K padding
  2. a natural 8-bit image (exact ties, near-ties): every query within the derived gap tau of the true minimum, every
     distance within (K + 4) 2^-24 relative
  3. the tie rule (smallest idx) and admissibility (ref_valid)
  4. wrap on one axis at a time, query only and reference only
  5. batches: row b is the B = 1 call on b's tensors, bit for bit; two runs are bit-equal
  6. the smallest grids
  7. patch_report and MultiscaleTrainer.evaluate
"""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import nnf_util as U
from conftest import GOLDEN
from sinddm_amd._lib import SinddmError
from sinddm_amd.synth import closed_form_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PS = (3, 5, 7)


def _nnf(q, r, P, wq=(False, False), wr=(False, False), valid=None):
    """numpy (B?, 3, H, W) -> (dist (B, h, w), idx (B, h, w)) numpy, through metrics.patch_nnf."""
    from sinddm_amd.metrics import patch_nnf
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)
    q, r = t(q), t(r)
    q = q[None] if q.dim() == 3 else q
    r = r[None] if r.dim() == 3 else r
    dist, yx = patch_nnf(q, r, P, wrap_query=wq, wrap_ref=wr, ref_valid=None if valid is None else t(valid))
    wr_ = U.grid(r.shape[2:], P, wr)[1]
    assert dist.dtype == torch.float32 and yx.dtype == torch.int32 and yx.shape == (dist.shape[0], 2) + dist.shape[1:]
    assert dist.shape[1:] == U.grid(q.shape[2:], P, wq)
    return dist.cpu().numpy(), (yx[:, 0].long() * wr_ + yx[:, 1].long()).cpu().numpy()


@pytest.fixture(scope="module")
def crops():
    img = np.asarray(Image.open(os.path.join(GOLDEN, "balloons.png")).convert("RGB"), dtype=np.float32)
    img = img.transpose(2, 0, 1) / 255.0 * 2.0 - 1.0
    q, r = img[:, 10:50, 20:72].copy(), img[:, 60:105, 100:137].copy()
    q.setflags(write=False)
    r.setflags(write=False)
    return q, r


@pytest.mark.parametrize("wrap", [(False, False), (True, True)], ids=["plain", "wrapxy"])
@pytest.mark.parametrize("P", PS)
def test_self_field_is_the_identity(P, wrap):
    x = np.random.default_rng(11).uniform(-1.0, 1.0, (3, 29, 37)).astype(np.float32)
    dist, idx = _nnf(x, x, P, wrap, wrap)
    h, w = U.grid((29, 37), P, wrap)
    assert idx.shape == (1, h, w)
    assert np.array_equal(idx.reshape(-1), np.arange(h * w)), int((idx.reshape(-1) != np.arange(h * w)).sum())
    assert (dist == 0.0).all(), float(np.abs(dist).max())


@pytest.mark.parametrize("P", PS)
def test_natural_image_against_brute_force(crops, P):
    q, r = crops
    dist, idx = _nnf(q, r, P)
    U.check_field(q, r, P, idx[0], dist[0], what=f"balloons P={P}")


def test_tie_rule_smallest_index():
    q = np.random.default_rng(5).uniform(-1.0, 1.0, (3, 21, 26)).astype(np.float32)
    r = np.full((3, 19, 23), 0.25, np.float32)
    for P in PS:
        _, idx = _nnf(q, r, P)
        assert (idx == 0).all(), (P, np.unique(idx))
        valid = np.ones((19, 23), np.float32)
        valid[:3] = 0.0                                        # the first admissible patch starts at row 3
        _, idx = _nnf(q, r, P, valid=valid)
        wr = 23 - P + 1
        assert (idx == 3 * wr).all(), (P, np.unique(idx))


@pytest.mark.parametrize("P", PS)
def test_hole_in_the_reference(crops, P):
    q, r = crops
    valid = np.ones(r.shape[1:], np.float32)
    valid[14:26, 11:20] = 0.0                                  # a 12 x 9 hole
    dist, idx = _nnf(q, r, P, valid=valid)
    ok = U.position_ok(valid, P)
    wr = r.shape[2] - P + 1
    y, x = idx[0] // wr, idx[0] % wr
    assert not ((y + P > 14) & (y < 26) & (x + P > 11) & (x < 20)).any()       # no winner's patch touches the hole
    U.check_field(q, r, P, idx[0], dist[0], ok=ok, what=f"balloons hole P={P}")


def test_empty_admissible_set_is_an_error(crops):
    q, r = crops
    with pytest.raises(SinddmError, match="no admissible"):
        _nnf(q, r, 7, valid=np.zeros(r.shape[1:], np.float32))


@pytest.mark.parametrize("side", ["query", "ref"])
@pytest.mark.parametrize("axis", [0, 1], ids=["y", "x"])
@pytest.mark.parametrize("P", (3, 7))
def test_wrap_on_one_axis(crops, P, axis, side):
    q, r = crops
    wrap = (axis == 0, axis == 1)
    wq, wr = (wrap, (False, False)) if side == "query" else ((False, False), wrap)
    dist, idx = _nnf(q, r, P, wq, wr)
    U.check_field(q, r, P, idx[0], dist[0], wrap_q=wq, wrap_r=wr, what=f"balloons wrap {side} {'yx'[axis]} P={P}")


def test_batch_rows_are_the_single_calls(crops):
    q, r = crops
    P = 5
    rng = np.random.default_rng(2)
    qs = np.stack([q, q[:, ::-1].copy(), np.clip(q + rng.normal(0, 0.05, q.shape), -1, 1).astype(np.float32)])
    rs = np.stack([r, r[:, :, ::-1].copy(), np.clip(r + rng.normal(0, 0.05, r.shape), -1, 1).astype(np.float32)])
    # B queries, one shared reference
    dist, idx = _nnf(qs, r, P, wq=(False, True))
    again = _nnf(qs, r, P, wq=(False, True))
    assert np.array_equal(dist.view(np.int32), again[0].view(np.int32)) and np.array_equal(idx, again[1])
    for b in range(3):
        d1, i1 = _nnf(qs[b], r, P, wq=(False, True))
        assert np.array_equal(i1[0], idx[b]) and np.array_equal(d1[0].view(np.int32), dist[b].view(np.int32)), b
    U.check_field(qs[2], r, P, idx[2], dist[2], wrap_q=(False, True), what="batch row 2, shared reference")
    # one shared query, B references (the coverage direction)
    dist, idx = _nnf(q, rs, P, wr=(True, False))
    assert dist.shape[0] == 3
    for b in range(3):
        d1, i1 = _nnf(q, rs[b], P, wr=(True, False))
        assert np.array_equal(i1[0], idx[b]) and np.array_equal(d1[0].view(np.int32), dist[b].view(np.int32)), b
    U.check_field(q, rs[1], P, idx[1], dist[1], wrap_r=(True, False), what="batch row 1, shared query")
    # both per sample
    dist, idx = _nnf(qs, rs, P)
    d1, i1 = _nnf(qs[1], rs[1], P)
    assert np.array_equal(i1[0], idx[1]) and np.array_equal(d1[0].view(np.int32), dist[1].view(np.int32))


def test_smallest_grids():
    rng = np.random.default_rng(8)
    q, r = rng.uniform(-1, 1, (3, 7, 7)).astype(np.float32), rng.uniform(-1, 1, (3, 7, 9)).astype(np.float32)
    dist, idx = _nnf(q, r, 7)                                   # one query position, 1 x 3 reference positions
    assert dist.shape == (1, 1, 1)
    U.check_field(q, r, 7, idx[0], dist[0], what="7x7 against 7x9")
    q, r = rng.uniform(-1, 1, (3, 12, 13)).astype(np.float32), rng.uniform(-1, 1, (3, 3, 19)).astype(np.float32)
    dist, idx = _nnf(q, r, 3)                                   # 17 reference positions: one more than an MFMA tile
    U.check_field(q, r, 3, idx[0], dist[0], what="17 reference positions")
    # ... of which the last one is the answer
    q2 = np.ascontiguousarray(r[:, :, 16:19])
    dist, idx = _nnf(q2, r, 3)
    assert idx.reshape(-1).tolist() == [16] and float(dist.reshape(-1)[0]) == 0.0
    # several 64-position chunks per row and a last partial one, several rows: 3 x 150 positions
    q, r = rng.uniform(-1, 1, (3, 9, 11)).astype(np.float32), rng.uniform(-1, 1, (3, 7, 154)).astype(np.float32)
    dist, idx = _nnf(q, r, 5)
    U.check_field(q, r, 5, idx[0], dist[0], what="3 x 150 positions")


def _trainer(golden, tmp_path, dim=32, T=20, batch=2):                     # the C1 recipe of tests/test_gpu_e2e.py
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    from sinddm_amd.trainer import MultiscaleTrainer
    meta = golden("g11_img_scales.json")["C1"]
    pyr = golden("c1_pyramid.npz")
    folder = str(tmp_path / "balloons") + "/"
    for key in pyr.files:
        os.makedirs(folder + key, exist_ok=True)
        Image.fromarray(pyr[key]).save(folder + key + "/balloons.png")
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    net.load_state_dict(closed_form_state_dict(dim))
    sizes = [tuple(s) for s in meta["sizes"]]
    d = MultiScaleGaussianDiffusion(net, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"], image_sizes=sizes,
                                    timesteps=T, train_full_t=True, scale_losses=meta["rescale_losses"], loss_factor=1,
                                    loss_type="l1", device=DEV, reblurring=True, omega=0,
                                    results_folder=str(tmp_path / "res")).to(DEV)
    tr = MultiscaleTrainer(d, folder=folder, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"],
                           image_sizes=sizes, train_batch_size=batch, train_lr=1e-3, train_num_steps=6,
                           gradient_accumulate_every=1, step_start_ema=2, update_ema_every=2,
                           save_and_sample_every=10 ** 9, avg_window=2, sched_milestones=[3],
                           results_folder=str(tmp_path / "res"), device=DEV)
    return tr, meta


def test_drivers(golden, tmp_path):
    from sinddm_amd.metrics import patch_report
    tr, meta = _trainer(golden, tmp_path)
    top = tr.n_scales - 1
    image = tr.data_list[top][0][0]
    rep = patch_report(image[None].repeat(2, 1, 1, 1).contiguous(), image)
    assert rep["fidelity"] == [0.0, 0.0] and rep["coverage"] == [0.0, 0.0] and rep["coherence"] == [1.0, 1.0]
    assert rep["fidelity_mean"] == 0.0 and rep["coherence_mean"] == 1.0 and "seam" not in rep
    # evaluate: draws its own batch with a few steps per scale, compares the finest scale, writes the report
    em = tr.ema_model
    em.sample_steps = 2
    torch.manual_seed(4)
    rep = tr.evaluate(batch_size=2, patch=5, custom_t_list=em.num_timesteps_ideal[1:])
    assert rep["scale"] == top and rep["patch"] == 5 and rep["samples"] == 2 and "seam" not in rep
    for key in ("fidelity", "coherence", "coverage"):
        assert len(rep[key]) == 2 and np.isfinite(rep[key]).all() and np.isfinite(rep[key + "_mean"]), key
    assert min(rep["fidelity"]) > 0.0 and 0.0 <= min(rep["coherence"]) <= max(rep["coherence"]) <= 1.0
    with open(os.path.join(str(tmp_path / "res"), "patch_report.json")) as f:
        assert json.load(f) == rep
    # a tiled sampler has a seam to report; given samples are scored as they are, at a coarser scale too
    em.tile = (False, True)
    outs = tr.sample_scales(batch_size=2, custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    rep = tr.evaluate(samples=outs, scale=1, patch=7)
    assert rep["scale"] == 1 and rep["tile"] == [False, True] and len(rep["seam"]) == 2
    for key in ("fidelity", "coherence", "coverage", "seam"):
        assert np.isfinite(rep[key]).all() and np.isfinite(rep[key + "_mean"]), key
    assert rep["sample_size"] == list(outs[1].shape[2:])
