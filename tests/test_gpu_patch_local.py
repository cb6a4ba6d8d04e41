"""GPU: the windowed patch search (sinddm_patch_nnf_local, csrc/patch_local.h) against the float64 window brute force of
tests/local_util.py, and the drivers that carry a field from iteration to iteration and from scale to scale.

  1. the field against float64: every P, radii 0 / 1 / 4 / 16, every wrap combination; random priors, priors on the corners
     and edges (clipped windows), windows that straddle x = 64 and the row end of the wide reference
  2. consistency with the exhaustive entry: bit-equal dist where the winners agree; a window that covers the grid
  3. exact cases: a copied patch gives 0.0, a constant reference gives the smallest index of the window
  4. admissibility and missing priors   5. the scaled ranking   6. equal bits: run = run, batch rows = single calls
  7. refusals   8. patch_refine(radius=...)   9. sample_scales(patch_refine={..., 'radius': R})
"""
import numpy as np
import pytest
import torch

import local_util as L
import nnf_util as U
import refine_util as R
from conftest import GOLDEN
from sinddm_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLAIN = (False, False)
INT32_MAX = 2 ** 31 - 1
GEOMETRIES = {"plain": (PLAIN, PLAIN), "wrapxy": ((True, True), PLAIN), "wrapy": ((True, False), PLAIN),
              "wrapx": ((False, True), PLAIN), "wrapref": (PLAIN, (True, True))}


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def _b(t):
    return t[None] if t.dim() == 3 else t


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _lin(yx, wr):
    return (yx[:, 0].long() * wr + yx[:, 1].long()).cpu().numpy()


def _nnf(q, r, P, wq=PLAIN, wr=PLAIN, valid=None):
    from sinddm_amd.metrics import patch_nnf
    dist, yx = patch_nnf(_b(_t(q)), _b(_t(r)), P, wrap_query=wq, wrap_ref=wr, ref_valid=None if valid is None else _t(valid))
    return dist.cpu().numpy(), _lin(yx, U.grid(np.shape(r)[-2:], P, wr)[1])


def _local(q, r, prior, radius, P, wq=PLAIN, wr=PLAIN, valid=None, scale=None):
    """numpy -> (dist (B, h, w), idx (B, h, w)) numpy through metrics.patch_nnf_local; prior (B, h, w) linear."""
    from sinddm_amd.metrics import patch_nnf_local
    dist, yx = patch_nnf_local(_b(_t(q)), _b(_t(r)), _t(prior, np.int32), radius, P, wrap_query=wq, wrap_ref=wr,
                               ref_valid=None if valid is None else _t(valid), ref_scale=None if scale is None else _t(scale))
    assert dist.dtype == torch.float32 and yx.dtype == torch.int32
    return dist.cpu().numpy(), _lin(yx, U.grid(np.shape(r)[-2:], P, wr)[1])


@pytest.fixture(scope="module")
def crops():
    return R.inputs(GOLDEN)


def _border_priors(qgrid, rgrid):
    """One prior per query, cycling over the four corners and the edge positions of the reference grid."""
    hr, wr = rgrid
    ys, xs = np.mgrid[0:hr, 0:wr]
    edge = (ys == 0) | (ys == hr - 1) | (xs == 0) | (xs == wr - 1)
    border = np.concatenate([[0, wr - 1, (hr - 1) * wr, hr * wr - 1], (ys * wr + xs)[edge]])
    return np.resize(border, qgrid[0] * qgrid[1]).reshape(qgrid)


# ---- 1. the field against float64 ----

@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("radius", (0, 1, 4, 16))
@pytest.mark.parametrize("P", (3, 5, 7))
def test_field_against_float64(crops, P, radius, geo):
    q, r, wide = crops
    wq, wr = GEOMETRIES[geo]
    rng = np.random.default_rng(100 * P + radius)
    qg = U.grid(q.shape[1:], P, wq)
    rg = U.grid(r.shape[1:], P, wr)
    priors = np.stack([rng.integers(0, rg[0] * rg[1], qg), _border_priors(qg, rg)])
    dist, idx = _local(q, r, priors, radius, P, wq, wr)
    for b, name in enumerate(("random", "corners and edges")):
        L.check_local_field(q, r, P, priors[b], radius, idx[b], dist[b], wq, wr, what=f"{name}, P={P} R={radius} {geo}")
    # the wide reference: windows around x = 64 and at the end of a row
    wg = U.grid(wide.shape[1:], P, wr)
    py = rng.integers(0, wg[0], qg)
    near64 = py * wg[1] + rng.integers(64 - radius - 1, 64 + radius + 2, qg).clip(0, wg[1] - 1)
    row_end = py * wg[1] + (wg[1] - 1 - rng.integers(0, radius + 2, qg)).clip(0, wg[1] - 1)
    priors = np.stack([near64, row_end])
    dist, idx = _local(q, wide, priors, radius, P, wq, wr)
    for b, name in enumerate(("around x = 64", "row end")):
        L.check_local_field(q, wide, P, priors[b], radius, idx[b], dist[b], wq, wr, what=f"wide, {name}, P={P} R={radius} {geo}")


# ---- 2. consistency with the exhaustive entry ----

@pytest.mark.parametrize("P", (3, 5, 7))
def test_consistency_with_the_exhaustive_entry(crops, P):
    q, r, wide = crops
    for ref, wq, wr in ((r, PLAIN, PLAIN), (wide, (False, True), PLAIN), (r, PLAIN, (True, True))):
        d0, i0 = _nnf(q, ref, P, wq, wr)
        for radius in (0, 2, 7, 16):
            d1, i1 = _local(q, ref, i0, radius, P, wq, wr)
            same = i0 == i1
            print(f"P={P} R={radius} ref {ref.shape[1:]}: {int((~same).sum())} of {same.size} winners differ")
            assert np.array_equal(_bits(d0[same]), _bits(d1[same]))
            if radius == 0:
                assert same.all()
            if not same.all():                                 # criterion 1 for both winners
                L.check_local_field(q, ref, P, i0[0], radius, i1[0], d1[0], wq, wr, what="local winners")
                L.check_local_field(q, ref, P, i0[0], radius, i0[0], d0[0], wq, wr, what="exhaustive winners")
    if P == 7:
        # a centre prior and R = 12 on the 24 x 30 reference: the window covers the whole 18 x 24 grid
        hr, wr_ = U.grid(r.shape[1:], P, PLAIN)
        assert (hr, wr_) == (18, 24)
        prior = np.full((1,) + U.grid(q.shape[1:], P, PLAIN), 9 * wr_ + 12)
        assert L.window_mask(prior[0], 12, (hr, wr_)).all()
        d1, i1 = _local(q, r, prior, 12, P)
        L.check_local_field(q, r, P, prior[0], 12, i1[0], d1[0], what="the window covers the grid")
        full = R.field64(q, r, P)[1]
        sel = full[np.arange(i1[0].size), i1[0].reshape(-1)]
        assert (sel - full.min(axis=1) <= (3 * P * P + 4) * R.U24 * (sel + full.min(axis=1))).all()


# ---- 3. exact cases ----

@pytest.mark.parametrize("P", (3, 5, 7))
def test_copied_patches_give_zero(crops, P):
    _, r, _ = crops
    q = r[:, 1:23, 2:28].copy()                                # query patch (y, x) is reference patch (y + 1, x + 2)
    qg, rg = U.grid(q.shape[1:], P, PLAIN), U.grid(r.shape[1:], P, PLAIN)
    yy, xx = np.mgrid[0:qg[0], 0:qg[1]]
    true = (yy + 1) * rg[1] + xx + 2
    rng = np.random.default_rng(P)
    for radius in (0, 3, 16):
        jy, jx = rng.integers(-radius, radius + 1, qg), rng.integers(-radius, radius + 1, qg)
        prior = np.clip(yy + 1 + jy, 0, rg[0] - 1) * rg[1] + np.clip(xx + 2 + jx, 0, rg[1] - 1)
        dist, idx = _local(q, r, prior[None], radius, P)
        assert (dist == 0.0).all()
        assert (idx[0] <= true).all()                          # that position, or a tied smaller one
        Bm = U.patches(r, P)[0]
        assert np.array_equal(Bm[idx[0].reshape(-1)], Bm[true.reshape(-1)])


def test_constant_reference_gives_the_smallest_index_of_the_window(crops):
    q, _, _ = crops
    P = 5
    rng = np.random.default_rng(0)
    qg = U.grid(q.shape[1:], P, PLAIN)
    for shape, wr, radius in (((3, 24, 30), PLAIN, 4), ((3, 24, 30), (True, True), 4), ((3, 9, 11), (True, True), 8),
                              ((3, 9, 40), (True, False), 16)):
        ref = np.full(shape, 0.25, np.float32)
        rg = U.grid(shape[1:], P, wr)
        prior = rng.integers(0, rg[0] * rg[1], qg)
        dist, idx = _local(q, ref, prior[None], radius, P, wr=wr)
        want = L.window_mask(prior, radius, rg, wr).argmax(axis=1)          # the first position of every window
        assert np.array_equal(idx[0].reshape(-1), want), (shape, wr, radius)
        if shape == (3, 9, 11):
            assert (idx == 0).all()                            # the window folds onto itself and covers the grid
        assert np.array_equal(_bits(dist), _bits(_local(q, ref, idx, 0, P, wr=wr)[0]))


# ---- 4. admissibility and missing priors ----

@pytest.mark.parametrize("P", (3, 5, 7))
def test_holes_and_missing_priors(crops, P):
    q, r, _ = crops
    valid = np.ones(r.shape[1:], np.float32)
    valid[8:15, 11:20] = 0.0
    ok = U.position_ok(valid, P)
    qg, rg = U.grid(q.shape[1:], P, PLAIN), U.grid(r.shape[1:], P, PLAIN)
    N = rg[0] * rg[1]
    rng = np.random.default_rng(P)
    prior = rng.integers(0, N, qg)
    prior[0, :3] = (-1, N, INT32_MAX)
    prior[1, :4] = 10 * rg[1] + 14                             # deep in the hole: with R = 1 no candidate is admissible
    assert not ok.reshape(rg)[9:12, 13:16].any()
    for radius in (1, 4):
        dist, idx = _local(q, r, prior[None], radius, P, valid=valid)
        L.check_local_field(q, r, P, prior, radius, idx[0], dist[0], ok=ok, what=f"hole, P={P} R={radius}")
        assert ok[idx[0][idx[0] >= 0]].all()                   # no winner touches the hole
        assert (idx[0, 0, :3] == -1).all() and np.isposinf(dist[0, 0, :3]).all()
        if radius == 1:
            assert (idx[0, 1, :4] == -1).all() and np.isposinf(dist[0, 1, :4]).all()
    # a field of missing priors only: the call returns 0 and reads nothing
    none = np.stack([np.full(qg, -1), np.full(qg, N), np.full(qg, INT32_MAX)])
    dist, idx = _local(q, r, none, 16, P)
    assert (idx == -1).all() and np.isposinf(dist).all()
    # coordinates: a (-1, .) pair is the linear position -1
    from sinddm_amd.metrics import patch_nnf_local
    pl = _t(prior, np.int32)
    yx = torch.stack([torch.div(pl, rg[1], rounding_mode="floor"), pl % rg[1]])[None].clone()
    yx[0, :, 0, 0] = torch.tensor([-1, rg[1] - 1], dtype=torch.int32)
    yx[0, :, 0, 1] = torch.tensor([0, rg[1]], dtype=torch.int32)            # a column past the grid: no prior either
    d2, yx2 = patch_nnf_local(_t(q)[None], _t(r)[None], yx.to(torch.int32), 4, P, ref_valid=_t(valid))
    d1, i1 = _local(q, r, prior[None], 4, P, valid=valid)
    assert np.array_equal(_bits(d2.cpu().numpy()), _bits(d1)) and np.array_equal(_lin(yx2, rg[1]), i1)


# ---- 5. the scale ----

@pytest.mark.parametrize("P", (3, 5, 7))
def test_scaled_field_against_float64(crops, P):
    q, r, wide = crops
    rng = np.random.default_rng(P)
    for ref in (r, wide):
        s = R.completeness_scale(q, ref, P)
        qg, rg = U.grid(q.shape[1:], P, PLAIN), U.grid(ref.shape[1:], P, PLAIN)
        prior = rng.integers(0, rg[0] * rg[1], qg)
        changed = 0
        for radius in (1, 4, 16):
            dist, idx = _local(q, ref, prior[None], radius, P, scale=s)
            L.check_local_field(q, ref, P, prior, radius, idx[0], dist[0], scale=s.reshape(-1),
                                what=f"scaled, ref {ref.shape[1:]}, P={P} R={radius}")
            changed += int((idx != _local(q, ref, prior[None], radius, P)[1]).sum())
        assert changed > 0                                     # the scale decides somewhere


# ---- 6. equal bits ----

def test_runs_and_batch_rows_are_equal_bits(crops):
    q, r, wide = crops
    P, radius, wq = 5, 4, (False, True)
    qs = np.stack([q, q[:, ::-1].copy(), q[:, :, ::-1].copy()])
    rs = np.stack([r, r[:, ::-1].copy(), r[:, :, ::-1].copy()])
    qg, rg = U.grid(q.shape[1:], P, wq), U.grid(r.shape[1:], P, PLAIN)
    priors = np.random.default_rng(6).integers(0, rg[0] * rg[1], (3,) + qg)
    ss = np.stack([R.completeness_scale(qs[b], r, P, wrap_q=wq) for b in range(3)])
    for ref, scale in ((r, None), (rs, None), (r, ss[0]), (r, ss), (rs, ss)):
        dist, idx = _local(qs, ref, priors, radius, P, wq, scale=scale)
        again = _local(qs, ref, priors, radius, P, wq, scale=scale)
        assert np.array_equal(_bits(dist), _bits(again[0])) and np.array_equal(idx, again[1])
        for b in range(3):
            d1, i1 = _local(qs[b], ref if ref.ndim == 3 else ref[b], priors[b:b + 1], radius, P, wq,
                            scale=scale if scale is None or scale.ndim == 2 else scale[b])
            assert np.array_equal(i1[0], idx[b]) and np.array_equal(_bits(d1[0]), _bits(dist[b])), b
    # a shared query against references per sample
    d, i = _local(q, rs, priors, radius, P, wq)
    d1, i1 = _local(q, rs[2], priors[2:3], radius, P, wq)
    assert np.array_equal(i1[0], i[2]) and np.array_equal(_bits(d1[0]), _bits(d[2]))


# ---- 7. refusals ----

def test_refusals(crops):
    from sinddm_amd.metrics import patch_nnf_local
    q, r, _ = crops
    P = 5
    x, ref = _t(q)[None].contiguous(), _t(r)[None].contiguous()
    qg, rg = U.grid(q.shape[1:], P, PLAIN), U.grid(r.shape[1:], P, PLAIN)
    prior = torch.zeros((1,) + qg, dtype=torch.int32, device=DEV)
    dist = torch.empty((1,) + qg, dtype=torch.float32, device=DEV)
    idx = torch.empty((1,) + qg, dtype=torch.int32, device=DEV)
    lib = _lib.load()

    def call(query=x.data_ptr(), ref_=ref.data_ptr(), prior_=prior.data_ptr(), dist_=dist.data_ptr(), idx_=idx.data_ptr(), B=1,
             Hq=q.shape[1], Wq=q.shape[2], Hr=r.shape[1], Wr=r.shape[2], P=P, radius=4):
        return lib.sinddm_patch_nnf_local(query, 1, ref_, 0, None, None, 0, prior_, radius, dist_, idx_, B, Hq, Wq, Hr, Wr, P, 0, 0,
                                          _lib.stream_ptr(x.device))

    assert call() == 0
    for kw in (dict(query=None), dict(ref_=None), dict(prior_=None), dict(dist_=None), dict(idx_=None), dict(B=0), dict(P=4),
               dict(P=9), dict(radius=-1), dict(radius=17)):
        assert call(**kw) == -1, kw
    for kw in (dict(Hq=4), dict(Wq=3), dict(Hr=2), dict(Wr=4), dict(Hr=50000, Wr=50000), dict(Hq=50000, Wq=50000)):
        assert call(**kw) == -2, kw
    E = _lib.SinddmError
    with pytest.raises(E, match="prior"):
        patch_nnf_local(x, ref, prior[:, :-1], 4, P)
    with pytest.raises(E, match="prior"):
        patch_nnf_local(x, ref, prior.long(), 4, P)
    with pytest.raises(E, match="radius"):
        patch_nnf_local(x, ref, prior, 17, P)
    with pytest.raises(E, match="patch"):
        patch_nnf_local(x, ref, prior, 4, 4)


# ---- 8. the loop ----

@pytest.mark.parametrize("tile", [PLAIN, (False, True)], ids=["plain", "tilex"])
def test_patch_refine_with_a_radius(crops, tile):
    from sinddm_amd.metrics import patch_nnf, patch_nnf_local
    from sinddm_amd.refine import patch_refine
    q, r, _ = crops
    P, radius = 5, 4
    x0 = _t(np.stack([q, q[:, ::-1].copy()]))
    image = _t(r)
    x, energy, hist, yx = patch_refine(x0, image, patch=P, iters=3, radius=radius, tile=tile, history=True, field=True)
    assert len(hist) == 3 and energy.shape == (3, 2) and energy.dtype == torch.float64 and torch.equal(x, hist[-1])
    wr = r.shape[2] - P + 1
    prev, field = x0, None
    for k in range(3):                                         # iteration 1 exhaustive, 2 and 3 windowed around the last field
        if k == 0:
            dist, field = patch_nnf(prev, image[None], P, wrap_query=tile)
        else:
            dist, field = patch_nnf_local(prev, image[None], field, radius, P, wrap_query=tile)
        assert torch.equal(dist.double().sum(dim=(1, 2)), energy[k]), k
        idx = _lin(field, wr)
        for b in range(2):                                     # the vote of the field the library returned, bit for bit
            want = R.vote_f32(idx[b], r, prev[b].cpu().numpy(), P, tile)
            assert np.array_equal(_bits(hist[k][b].cpu().numpy()), _bits(want)), (k, b)
        prev = hist[k]
    assert torch.equal(field, yx)
    e = energy.cpu().numpy()
    print(f"tile={tile}: energies " + " | ".join(" -> ".join(f"{v:.6g}" for v in e[:, b]) for b in range(2)))
    for k in range(2):                                         # the window contains the previous assignment: no rise
        assert (e[k + 1] <= e[k] * (1.0 + 3 * P * P * 2.0 ** -23)).all(), (k, e)
    # radius = None is the call as it was: the bits of a call without the keyword
    a = patch_refine(x0, image, patch=P, iters=2, tile=tile, radius=None, prior=None, field=False)
    b_ = patch_refine(x0, image, patch=P, iters=2, tile=tile)
    assert len(a) == len(b_) == 2 and torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    # a prior for the first iteration: the exhaustive field itself as prior gives the first iterate again
    d0, f0 = patch_nnf(x0, image[None], P, wrap_query=tile)
    given = patch_refine(x0, image, patch=P, iters=1, radius=0, prior=f0, tile=tile, field=True)
    assert torch.equal(given[0], hist[0]) and torch.equal(given[1], energy[:1]) and torch.equal(given[2], f0)
    # queries without a prior are skipped by the vote and add nothing to the energy
    holes = f0.clone()
    holes[:, 0, 2:9, 3:12] = -1
    holes[:, 1, 2:9, 3:12] = wr - 1
    part = patch_refine(x0, image, patch=P, iters=1, radius=0, prior=holes, tile=tile, field=True)
    keep = torch.ones_like(d0, dtype=torch.bool)
    keep[:, 2:9, 3:12] = False
    assert torch.equal(part[1][0], (d0.double() * keep).sum(dim=(1, 2))) and bool((part[2][:, 0][~keep] == -1).all())
    assert torch.equal(part[0][:, :, 6, 7 + P - 1], x0[:, :, 6, 7 + P - 1])      # a pixel only skipped patches cover


# ---- 9. the pyramid ----

def test_pyramid_driver_carries_the_field(golden, tmp_path):
    from sinddm_amd.refine import carry_field
    from test_gpu_patch_nnf import _trainer
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    em.sample_steps = 2
    assert tr.n_scales == 3
    t_list = em.num_timesteps_ideal[1:]
    kw = dict(batch_size=2, custom_t_list=t_list, save_images=False, seeds=[5, 6])
    opt = {"iters": 1, "patch": 5, "scales": (1, 2), "radius": 4}
    on = tr.sample_scales(patch_refine=opt, **kw)
    sizes = [tuple(s)[::-1] for s in meta["sizes"]]             # (the recipe lists (W, H))
    assert [tuple(b.shape) for b in on] == [(2, 3) + s for s in sizes] and all(bool(torch.isfinite(b).all()) for b in on)
    again = tr.sample_scales(patch_refine=dict(opt), **kw)
    assert all(torch.equal(a, b) for a, b in zip(on, again))
    # by hand: chain -> exhaustive refine at scale 1 -> carry_field -> chain -> windowed refine at scale 2
    images = [tr.data_list[s][0][0] for s in range(3)]
    with em.sampling(**tr._call_options([5, 6], None, None, 2, sharded=True)):
        c0 = em.sample(batch_size=2, scale_0_size=None, s=0)
        c1 = em.sample_via_scale(2, c0, s=1, scale_mul=(1, 1), custom_sample=False, custom_img_size_idx=1, custom_t=t_list[0])
        r1, _, f1 = tr.refine(c1, scale=1, patch=5, iters=1, radius=4, field=True)
        assert torch.equal(r1, tr.refine(c1, scale=1, patch=5, iters=1)[0])          # the first covered scale is exhaustive
        c2 = em.sample_via_scale(2, r1, s=2, scale_mul=(1, 1), custom_sample=False, custom_img_size_idx=2, custom_t=t_list[1])
        prior = carry_field(f1, 5, c1.shape[2:], c2.shape[2:], images[1].shape[1:], images[2].shape[1:])
        r2, e2, f2 = tr.refine(c2, scale=2, patch=5, iters=1, radius=4, prior=prior, field=True)
    assert torch.equal(on[0], c0) and torch.equal(on[1], r1) and torch.equal(on[2], r2)
    # the windowed field is a field of the window: every winner within 4 positions of its prior
    assert bool(((f2 - prior).abs() <= 4).all())
    full = tr.refine(c2, scale=2, patch=5, iters=1, field=True)
    share = float((full[2] == f2).all(dim=1).float().mean())
    print(f"scale 2: {share:.1%} of the windowed winners are the exhaustive ones; energy {e2.tolist()} vs {full[1].tolist()}")
    # without a radius the run is the run as it was
    plain = {k: v for k, v in opt.items() if k != "radius"}
    off = tr.sample_scales(patch_refine=plain, **kw)
    assert torch.equal(off[1], on[1]) and torch.equal(off[2], tr.refine(c2, scale=2, patch=5, iters=1)[0])
    none = tr.sample_scales(patch_refine=dict(plain, radius=None), **kw)
    assert all(torch.equal(a, b) for a, b in zip(off, none))
