"""GPU: the patch vote (csrc/patch_vote.h), the scaled patch field (sinddm_patch_nnf_scaled) and the refinement drivers
against the numpy references of tests/refine_util.py.

  1. the vote against a float32 emulation with the kernel's add order, bit for bit: plain, wrapped query axes, a wrapped
     reference, entries that name no patch, an uncovered pixel, batches, a single patch, in place
  2. the scaled field against float64 brute force of D_ij s_j, within the bound derived in refine_util.check_scaled_field
  3. what must be equal bits: no scale = sinddm_patch_nnf, batch rows = single calls, run = run
  4. patch_refine: every iterate is vote(field(previous)), the float64 energy of the iterates does not rise
  5. sample_scales(patch_refine=...), refine() and evaluate() on the C1 recipe
"""
import numpy as np
import pytest
import torch

import nnf_util as U
import refine_util as R
from conftest import GOLDEN
from sinddm_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLAIN = (False, False)


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def _b(t):
    return t[None] if t.dim() == 3 else t


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _nnf(q, r, P, wq=PLAIN, wr=PLAIN, valid=None, scale=None, **kw):
    """numpy -> (dist (B, h, w), idx (B, h, w)) numpy through metrics.patch_nnf."""
    from sinddm_amd.metrics import patch_nnf
    q, r = _b(_t(q)), _b(_t(r))
    if scale is not None:
        kw["ref_scale"] = _t(scale)
    dist, yx = patch_nnf(q, r, P, wrap_query=wq, wrap_ref=wr, ref_valid=None if valid is None else _t(valid), **kw)
    wr_ = U.grid(r.shape[2:], P, wr)[1]
    return dist.cpu().numpy(), (yx[:, 0].long() * wr_ + yx[:, 1].long()).cpu().numpy()


def _vote(idx, ref, base, P, wq=PLAIN, wr=PLAIN, weight=None, blend=1.0):
    from sinddm_amd.refine import patch_vote
    base = _b(_t(base))
    out = patch_vote(_t(idx, np.int32), _b(_t(ref)), base.shape[2:], P, wq, wr, base=base,
                     weight=None if weight is None else _t(weight), blend=blend)
    assert out.shape == base.shape and out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def crops():
    return R.inputs(GOLDEN)


def _weights(shape, seed):
    return np.random.default_rng(seed).choice(np.array([0.0, 0.25, 0.5, 1.0], np.float32), size=shape)


# ---- 1. the vote ----

GEOMETRIES = {"plain": (PLAIN, PLAIN), "wrapxy": ((True, True), PLAIN), "wrapy": ((True, False), PLAIN),
              "wrapx": ((False, True), PLAIN), "wrapref": (PLAIN, (True, True))}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("P", (3, 5, 7))
def test_vote_is_the_emulation_bit_for_bit(crops, P, geo):
    q, r, _ = crops
    wq, wr = GEOMETRIES[geo]
    _, idx = _nnf(q, r, P, wq, wr)
    idx = idx[0].copy()
    rng = np.random.default_rng(P)
    idx[rng.random(idx.shape) < 0.1] = -1                      # some entries name no patch
    w = _weights(q.shape[1:], 7)
    for blend, weight in ((1.0, None), (0.5, None), (1.0, w), (0.5, w)):
        out = _vote(idx[None], r, q, P, wq, wr, weight, blend)[0]
        want = R.vote_f32(idx, r, q, P, wq, wr, weight, blend)
        assert np.array_equal(_bits(out), _bits(want)), (blend, weight is not None, int((_bits(out) != _bits(want)).sum()))
        if weight is not None:
            assert np.array_equal(out[:, w == 0], q[:, w == 0])


def test_vote_uncovered_pixel_and_no_patch_at_all(crops):
    q, r, _ = crops
    P = 5
    _, idx = _nnf(q, r, P)
    idx = idx[0].copy()
    idx[4:4 + P, 9:9 + P] = -1                                 # pixel (8, 13) is covered by exactly these positions
    out = _vote(idx[None], r, q, P)[0]
    assert np.array_equal(_bits(out), _bits(R.vote_f32(idx, r, q, P)))
    assert np.array_equal(out[:, 8, 13], q[:, 8, 13])
    assert not np.array_equal(out[:, 8, 14], q[:, 8, 14])
    none = np.full_like(idx, -1)
    assert np.array_equal(_bits(_vote(none[None], r, q, P, blend=0.5)[0]), _bits(q))
    assert np.array_equal(_bits(_vote(idx[None], r, q, P, blend=0.0)[0]), _bits(q))


def test_vote_batches(crops):
    q, r, wide = crops
    P = 5
    qs = np.stack([q, q[:, ::-1].copy()])
    rs = np.stack([r, r[:, :, ::-1].copy()])
    ws = np.stack([_weights(q.shape[1:], 1), _weights(q.shape[1:], 2)])
    wq = (False, True)
    # a shared reference, a weight map per sample
    _, idx = _nnf(qs, r, P, wq)
    out = _vote(idx, r, qs, P, wq, weight=ws, blend=0.5)
    for b in range(2):
        assert np.array_equal(_bits(out[b]), _bits(R.vote_f32(idx[b], r, qs[b], P, wq, weight=ws[b], blend=0.5))), b
    # a reference per sample, one shared weight map
    _, idx = _nnf(qs, rs, P, wq)
    out = _vote(idx, rs, qs, P, wq, weight=ws[0])
    for b in range(2):
        assert np.array_equal(_bits(out[b]), _bits(R.vote_f32(idx[b], rs[b], qs[b], P, wq, weight=ws[0]))), b
    # more than one 32 x 8 tile in both directions, sizes that are no multiple of the tile
    _, idx = _nnf(wide, r, 7)
    out = _vote(idx, r, wide, 7)
    assert np.array_equal(_bits(out[0]), _bits(R.vote_f32(idx[0], r, wide, 7)))


@pytest.mark.parametrize("P", (3, 5, 7))
def test_vote_of_one_patch_is_the_patch_and_in_place(crops, P):
    q, r, _ = crops
    wr = r.shape[2] - P + 1
    n = 3 * wr + 4
    out = _vote(np.array([[[n]]]), r, q[:, :P, :P], P)[0]
    assert np.array_equal(_bits(out), _bits(r[:, 3:3 + P, 4:4 + P]))
    # in place through the C entry: out aliases base
    _, idx = _nnf(q, r, P)
    want = R.vote_f32(idx[0], r, q, P, blend=0.5)
    x, ref, field = _t(q)[None].contiguous(), _t(r)[None].contiguous(), _t(idx, np.int32).contiguous()
    rc = _lib.load().sinddm_patch_vote(field.data_ptr(), ref.data_ptr(), 0, x.data_ptr(), None, 0, x.data_ptr(), 1, q.shape[1],
                                       q.shape[2], r.shape[1], r.shape[2], P, 0, 0, 0.5, _lib.stream_ptr(x.device))
    assert rc == 0
    assert np.array_equal(_bits(x[0].cpu().numpy()), _bits(want))


# ---- 2. the scaled field ----

@pytest.mark.parametrize("P", (3, 5, 7))
def test_scaled_field_against_brute_force(crops, P):
    q, r, wide = crops
    qs = np.stack([q, q[:, ::-1].copy()])
    # one shared scale map, a reference row of two chunks (the second one partial), B = 2
    s = R.completeness_scale(q, wide, P)
    dist, idx = _nnf(qs, wide, P, scale=s)
    plain = _nnf(qs, wide, P)[1]
    assert (idx[0] != plain[0]).mean() >= 0.25                 # the scale decides (test_patch_refine_host: in float64 too)
    for b in range(2):
        R.check_scaled_field(qs[b], wide, P, s, idx[b], dist[b], what=f"shared scale, wide reference, row {b}, P={P}")
    # a scale map per sample
    ss = np.stack([R.completeness_scale(qs[b], r, P) for b in range(2)])
    dist, idx = _nnf(qs, r, P, scale=ss)
    for b in range(2):
        R.check_scaled_field(qs[b], r, P, ss[b], idx[b], dist[b], what=f"per-sample scale, row {b}, P={P}")
    assert not np.array_equal(idx[1], _nnf(qs[1], r, P, scale=ss[0])[1][0])    # (row 1 did use its own map)
    # a natural query without noise (exact ties and near-ties among its patches), several query tiles
    s = R.completeness_scale(wide, r, P)
    dist, idx = _nnf(wide, r, P, scale=s)
    R.check_scaled_field(wide, r, P, s, idx[0], dist[0], what=f"natural query, P={P}")
    # a hole in the reference
    valid = np.ones(r.shape[1:], np.float32)
    valid[8:15, 11:20] = 0.0
    ok = U.position_ok(valid, P)
    dist, idx = _nnf(q, r, P, valid=valid, scale=ss[0])
    R.check_scaled_field(q, r, P, ss[0], idx[0], dist[0], ok=ok, what=f"hole, P={P}")
    # wrapped axes: the query in x, the reference in y
    s = R.completeness_scale(q, r, P, wrap_q=(False, True))
    dist, idx = _nnf(q, r, P, wq=(False, True), scale=s)
    R.check_scaled_field(q, r, P, s, idx[0], dist[0], wrap_q=(False, True), what=f"query wraps in x, P={P}")
    A, _ = U.patches(r, P, (True, False))
    s = (1.0 / (R.ALPHA * 3 * P * P + U.distances(A, U.patches(q, P)[0]).min(axis=1))).astype(np.float32)
    s = s.reshape(U.grid(r.shape[1:], P, (True, False)))
    dist, idx = _nnf(q, r, P, wr=(True, False), scale=s)
    R.check_scaled_field(q, r, P, s, idx[0], dist[0], wrap_r=(True, False), what=f"reference wraps in y, P={P}")


# ---- 3. equal bits ----

def test_no_scale_is_the_plain_field_and_rows_are_single_calls(crops):
    q, r, wide = crops
    P = 5
    qs = np.stack([q, q[:, ::-1].copy(), q[:, :, ::-1].copy()])
    base = _nnf(qs, r, P, (False, True))
    none = _nnf(qs, r, P, (False, True), ref_scale=None)
    assert np.array_equal(_bits(base[0]), _bits(none[0])) and np.array_equal(base[1], none[1])
    # a NULL scale through the new C entry, with the new entry's workspace
    lib = _lib.load()
    x, ref = _t(qs).contiguous(), _t(r)[None].contiguous()
    B, (H, W), (Hr, Wr) = 3, q.shape[1:], r.shape[1:]
    h, w = U.grid((H, W), P, (False, True))
    nbytes = lib.sinddm_patch_nnf_scaled_workspace_bytes(B, H, W, Hr, Wr, P, 2, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dist = torch.empty(B, h, w, dtype=torch.float32, device=DEV)
    idx = torch.empty(B, h, w, dtype=torch.int32, device=DEV)
    rc = lib.sinddm_patch_nnf_scaled(x.data_ptr(), 1, ref.data_ptr(), 0, None, None, 0, dist.data_ptr(), idx.data_ptr(), B, H, W,
                                     Hr, Wr, P, 2, 0, ws.data_ptr(), nbytes, _lib.stream_ptr(x.device))
    assert rc == 0
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(base[0])) and np.array_equal(idx.cpu().numpy(), base[1])
    # scaled: rows of a batch are the single calls, shared and per-sample maps, and a second run gives the same bits
    for ref_img in (r, wide):
        ss = np.stack([R.completeness_scale(qs[b], ref_img, P, wrap_q=(False, True)) for b in range(3)])
        for scale in (ss[0], ss):
            dist, idx = _nnf(qs, ref_img, P, (False, True), scale=scale)
            again = _nnf(qs, ref_img, P, (False, True), scale=scale)
            assert np.array_equal(_bits(dist), _bits(again[0])) and np.array_equal(idx, again[1])
            for b in range(3):
                d1, i1 = _nnf(qs[b], ref_img, P, (False, True), scale=scale if scale.ndim == 2 else scale[b])
                assert np.array_equal(i1[0], idx[b]) and np.array_equal(_bits(d1[0]), _bits(dist[b])), b
    # both images per sample
    rs = np.stack([r, r[:, ::-1].copy(), r[:, :, ::-1].copy()])
    ss = np.stack([R.completeness_scale(qs[b], rs[b], P) for b in range(3)])
    dist, idx = _nnf(qs, rs, P, scale=ss)
    d1, i1 = _nnf(qs[2], rs[2], P, scale=ss[2])
    assert np.array_equal(i1[0], idx[2]) and np.array_equal(_bits(d1[0]), _bits(dist[2]))
    R.check_scaled_field(qs[2], rs[2], P, ss[2], idx[2], dist[2], what="both per sample, row 2")


def test_bad_scales_are_refused(crops):
    q, r, _ = crops
    s = R.completeness_scale(q, r, 5).copy()
    for bad in (0.0, -1.0, np.inf, np.nan):
        s2 = s.copy()
        s2[3, 4] = bad
        with pytest.raises(_lib.SinddmError, match="finite and > 0"):
            _nnf(q, r, 5, scale=s2)
    with pytest.raises(_lib.SinddmError, match="ref_scale"):
        _nnf(q, r, 5, scale=s[:, :-1])


# ---- 4. the driver ----

@pytest.mark.parametrize("blend", (1.0, 0.5))
@pytest.mark.parametrize("tile", [PLAIN, (True, True)], ids=["plain", "tilexy"])
@pytest.mark.parametrize("P", (5, 7))
def test_patch_refine_iterates_and_energy(crops, P, tile, blend):
    from sinddm_amd.metrics import patch_nnf
    from sinddm_amd.refine import patch_refine, patch_vote
    q, r, _ = crops
    x0 = _t(np.stack([q, q[:, ::-1].copy()]))
    image = _t(r)
    x, energy, hist = patch_refine(x0, image, patch=P, iters=3, blend=blend, tile=tile, history=True)
    assert len(hist) == 3 and energy.shape == (3, 2) and energy.dtype == torch.float64 and torch.equal(x, hist[-1])
    again = patch_refine(x0, image, patch=P, iters=3, blend=blend, tile=tile)
    assert len(again) == 2 and torch.equal(again[0], x) and torch.equal(again[1], energy)
    prev = x0
    for k in range(3):                                         # the driver adds no arithmetic
        dist, yx = patch_nnf(prev, image[None], P, wrap_query=tile)
        step = patch_vote(yx, image[None], prev.shape[2:], P, tile, PLAIN, base=prev, blend=blend)
        assert torch.equal(step, hist[k]), k
        assert torch.equal(dist.double().sum(dim=(1, 2)), energy[k]), k
        prev = step
    its = [x0.cpu().numpy()] + [h.cpu().numpy() for h in hist]
    for b in range(2):
        es = [R.energy64(it[b], r, P, tile) for it in its]     # (E*, sum of tau) of every iterate
        print(f"P={P} tile={tile} blend={blend} sample {b}: E* " + " -> ".join(f"{e:.5g}" for e, _ in es)
              + f" (sum tau {es[0][1]:.3g}); the field's own sums " + " ".join(f"{float(v):.5g}" for v in energy[:, b]))
        for k in range(3):
            assert es[k + 1][0] <= es[k][0] + es[k][1], (b, k, es)
            assert abs(float(energy[k, b]) - es[k][0]) <= es[k][1] + 1e-5 * es[k][0], (b, k)
        if blend == 1.0 and tile == PLAIN and b == 0:
            assert es[1][0] < es[0][0] / 100.0, es              # the noisy crop lands on the image's patches


def test_patch_refine_with_alpha_is_its_parts(crops):
    from sinddm_amd.metrics import patch_nnf
    from sinddm_amd.refine import patch_refine, patch_vote
    q, r, _ = crops
    P, tile = 5, (False, True)
    x0 = _t(np.stack([q, q[:, ::-1].copy()]))
    image = _t(r)[None]
    valid = np.ones(r.shape[1:], np.float32)
    valid[:6, :9] = 0.0
    x, energy, hist = patch_refine(x0, image[0], patch=P, iters=2, alpha=R.ALPHA, tile=tile, valid=_t(valid), history=True)
    prev = x0
    for k in range(2):
        m, _ = patch_nnf(image, prev, P, wrap_ref=tile)
        scale = 1.0 / (R.ALPHA * 3 * P * P + m)
        dist, yx = patch_nnf(prev, image, P, wrap_query=tile, ref_valid=_t(valid), ref_scale=scale)
        if k == 0:                                             # the float64 reference of the same scale agrees
            s64 = R.completeness_scale(q, r, P, wrap_q=tile)
            assert np.allclose(scale[0].cpu().numpy(), s64, rtol=1e-4, atol=0)
            wr = r.shape[2] - P + 1
            idx = (yx[0, 0].long() * wr + yx[0, 1]).cpu().numpy()
            R.check_scaled_field(q, r, P, scale[0].cpu().numpy(), idx, dist[0].cpu().numpy(), wrap_q=tile,
                                 ok=U.position_ok(valid, P), what="alpha, first iteration")
            y, xx = idx // wr, idx % wr
            assert not ((y < 6) & (xx < 9)).any()              # the hole is never copied from
        step = patch_vote(yx, image, prev.shape[2:], P, tile, PLAIN, base=prev)
        assert torch.equal(step, hist[k]) and torch.equal(dist.double().sum(dim=(1, 2)), energy[k]), k
        prev = step
    plain = patch_refine(x0, image[0], patch=P, iters=1, tile=tile, valid=_t(valid))[0]
    assert not torch.equal(plain, hist[0])


@pytest.mark.parametrize("P", (3, 5, 7))
def test_self_refinement_returns_the_image(crops, P):
    from sinddm_amd.refine import patch_refine
    _, r, wide = crops
    for img in (r, wide):
        x, energy = patch_refine(_t(img)[None], _t(img), patch=P, iters=1)
        assert float(energy.abs().max()) == 0.0                # every patch finds itself (or an identical one)
        err = np.abs(x[0].cpu().numpy().astype(np.float64) - img)
        # a pixel is the mean of up to P^2 equal values: P^2 - 1 roundings of the sum and one of the quotient
        assert (err <= (P * P + 1) * R.U24 * np.abs(img)).all(), float((err / np.maximum(np.abs(img), 1e-30)).max())


# ---- 5. the pyramid ----

def test_pyramid_drivers(golden, tmp_path):
    from sinddm_amd.refine import PatchRefine
    from test_gpu_patch_nnf import _trainer
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    em.sample_steps = 2
    top = tr.n_scales - 1
    kw = dict(batch_size=2, custom_t_list=em.num_timesteps_ideal[1:], save_images=False, seeds=[5, 6])
    off = tr.sample_scales(**kw)
    off2 = tr.sample_scales(patch_refine=None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(off, off2))   # without the option: the run as it was
    # the first refined scale is refine() of the unrefined run's batch; the scales before it are untouched
    on = tr.sample_scales(patch_refine=dict(iters=2, patch=5, scales=(1, top)), **kw)
    assert torch.equal(on[0], off[0])
    want, energy = tr.refine(off, scale=1, patch=5, iters=2)
    assert torch.equal(on[1], want) and not torch.equal(on[1], off[1])
    assert energy.shape == (2, 2) and bool((energy[1] <= energy[0]).all())
    assert not torch.equal(on[top], off[top])                  # ... and the later scales start from the refined one
    same = tr.sample_scales(patch_refine=PatchRefine(iters=2, patch=5, scales=(1, top)), **kw)
    assert all(torch.equal(a, b) for a, b in zip(on, same))
    # evaluate gets the option for free; refining the finest scale cannot make its fidelity worse (same patch size)
    P = 5
    ekw = {k: v for k, v in kw.items() if k != "save_images"}  # (evaluate never saves images)
    rep_off = tr.evaluate(patch=P, **ekw)
    rep_on = tr.evaluate(patch=P, patch_refine=dict(iters=1, patch=P, scales=(top, top)), **ekw)
    image = tr.data_list[top][0][0].cpu().numpy()
    A = [U.patches(x, P)[0] for x in off[top].cpu().numpy()]
    Bm = U.patches(image, P)[0]
    for b in range(2):
        tol = float(R.tau(A[b], Bm, P).mean()) / (3 * P * P)
        print(f"sample {b}: fidelity {rep_off['fidelity'][b]:.6g} -> {rep_on['fidelity'][b]:.6g} (tau {tol:.3g})")
        assert rep_on["fidelity"][b] <= rep_off["fidelity"][b] + tol, b
    assert rep_on["fidelity_mean"] < rep_off["fidelity_mean"]
    # tiled samples: the wrapped axes of the sampler are the wrapped axes of the vote
    em.tile = (False, True)
    try:
        t_off = tr.sample_scales(**kw)
        t_on = tr.sample_scales(patch_refine=dict(patch=5, scales=(top, top)), **kw)
        assert torch.equal(t_on[top], tr.refine(t_off, patch=5)[0]) and torch.equal(t_on[top - 1], t_off[top - 1])
    finally:
        em.tile = (False, False)
    # what is not built says so
    em.keep_maps = {}
    try:
        with pytest.raises(NotImplementedError, match="patch_refine with keep_maps"):
            tr.sample_scales(patch_refine=dict(iters=1), **kw)
    finally:
        em.keep_maps = None
    with pytest.raises(_lib.SinddmError, match="patch_refine"):
        tr.sample_scales(patch_refine=dict(scales=(2, 1)), **kw)
