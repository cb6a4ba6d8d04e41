"""Denoising-score maps on the GPU: sinddm_score_chain (include/sinddm_hip.h, csrc/score_tail.h) and
MultiScaleGaussianDiffusion.denoise_score / MultiscaleTrainer.score above it.

He-normal full-rank nets (sinddm_amd.synth.he_state_dict(dim), eps_gain 1: an untrained network, eps of rms ~10 ... 70), the C1
schedule of tests/golden (T = 100, 3 scales), 3 ... 5 evaluations per call.  The shapes are chosen by the ending they take,
and test_shapes_take_their_routes asserts it through sinddm_debug_forward_plan:

    dim 16, B 2, 12x16   aligned fused tail, last launch 1 (head + step)             the base case
    dim 16, B 3, 13x17   padded rows, last launch 0, a plane of 221 floats           every unaligned r0 of the two-call Philox draw
                                                                                     occurs (663 % 4 = 3 shifts it per sample,
                                                                                     17 % 4 = 1 per row), a row's last quad is cut
    dim 20, B 2, 13x17   fuse_tail == 0: eps through memory, score_rows_kernel       and a score_draw_kernel per evaluation
    dim 16, B 2, 40x52   aligned fused tail, three blocks per sample                 the level sums cross blocks

  1. x_t on return is sinddm_q_sample of the last evaluation's draw, bit for bit; NaN guard bands around every output
  2. the map and the table against float64 (tests/score_util.py), the yardstick being the composed route on the entries that
     existed before (sinddm_q_sample + sinddm_net_forward + torch abs / sum, same draws): error <= 2 E_c
  3. the level sums: within 1e-6 of the float64 sum of the fp32 map values, bit-equal run to run
  4. a weight plane with exact zeros; 5. per-sample seeds; 6. the level sums are the training loss (p_losses)
  7. a pasted 3x3 gray patch: the map's arg-max lies inside the patch dilated by 16 px (asserted; it is the clean crop's
     arg-max too), the map moves only within the receptive radius (asserted, bit for bit); the untrained net does not score
     the patch above the image mean (0.955 measured: printed, not asserted)
  8. error codes; 9. denoise_score and MultiscaleTrainer.score are this call, also under a train mask
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from score_util import dilate, level_sum_f64, score_f64
from sinddm_amd.synth import hash_randn
from test_fwd_plan_host import plan
from train_step_util import DEV, sched_and_diffusion

pytestmark = pytest.mark.gpu

SHAPES = [(16, 2, 12, 16), (16, 3, 13, 17), (20, 2, 13, 17), (16, 2, 40, 52)]
IDS = ["aligned", "padded", "rows", "blocks"]
SID0 = (2 << 32) | 0x40000000
_CACHE = {}


def _model(golden, dim):
    if dim not in _CACHE:
        _CACHE[dim] = sched_and_diffusion(golden, dim)
    return _CACHE[dim]


def _pics(B, H, W, key=900):
    y = hash_randn((B, 3, H, W), key + W).mul(0.5).clamp(-1, 1)
    yp = hash_randn((B, 3, H, W), key + 1 + W).mul(0.4).clamp(-1, 1)
    return y, yp


def _guarded(shape, guard=8):
    big = torch.full((guard + int(np.prod(shape)) + guard,), float("nan"), device=DEV)
    return big, big[guard:-guard].view(shape), guard


def _call(net, d, y, yp, s, t_list, seed=77, sid0=SID0, seeds=None, weight=None, ws_bytes=None, check=True):
    """One sinddm_score_chain call on device copies, every output inside NaN guard bands.  Returns (rc, x_t, map, level) on the
    CPU; the guards are checked here."""
    from sinddm_amd import _lib
    from sinddm_amd.models import _workspace
    lib = _lib.load()
    B, _, H, W = y.shape
    n = len(t_list)
    yd = y.to(DEV).contiguous()
    ypd = yp.to(DEV).contiguous() if s > 0 else None
    gx, xt, g = _guarded((B, 3, H, W))
    gm, smap, _ = _guarded((B, H, W))
    gl, lev, _ = _guarded((n, B))
    need = lib.sinddm_score_workspace_bytes(net.dim_arg, B, H, W, n)
    assert need >= lib.sinddm_workspace_bytes(net.dim_arg, B, H, W) > 0
    ws = _workspace(DEV, need)
    sd = torch.tensor(seeds, dtype=torch.int64, device=DEV) if seeds is not None else None
    wd = weight.to(DEV).contiguous() if weight is not None else None
    opts = _lib.ScoreOpts(_lib.ptr(wd), _lib.ptr(sd))
    gamma = d.gammas[s - 1].contiguous() if s > 0 else None
    tl = (C.c_int * n)(*t_list)
    rc = lib.sinddm_score_chain(_lib.ptr(net.flat_params), _lib.ptr(net.packed_weights()), _lib.ptr(yd), _lib.ptr(ypd),
                                xt.data_ptr(), _lib.ptr(d.sqrt_alphas_cumprod), _lib.ptr(d.sqrt_one_minus_alphas_cumprod),
                                _lib.ptr(gamma), tl, n, float(s), seed, sid0, smap.data_ptr(), lev.data_ptr(), net.dim_arg, B, H,
                                W, ws.data_ptr(), need if ws_bytes is None else ws_bytes, _lib.stream_ptr(DEV), C.byref(opts))
    torch.cuda.synchronize()
    for big in (gx, gm, gl):
        assert bool(big[:g].isnan().all()) and bool(big[-g:].isnan().all()), "an output ran over its guard band"
    if check:
        assert rc == 0
        assert not bool(xt.isnan().any()) and not bool(smap.isnan().any()) and not bool(lev.isnan().any())
    return rc, xt.cpu(), smap.cpu(), lev.cpu()


def _draws(B, H, W, n, seed=77, sid0=SID0, seeds=None):
    """The device's own z_i of a call, (n,B,3,H,W) on the device: sinddm_normal_fill of the whole batch, or with per-sample
    seeds sinddm_normal_fill_samples."""
    from sinddm_amd import _lib
    lib = _lib.load()
    z = torch.empty((n, B, 3, H, W), device=DEV)
    sd = torch.tensor(seeds, dtype=torch.int64, device=DEV) if seeds is not None else None
    for i in range(n):
        if sd is None:
            _lib.check(lib.sinddm_normal_fill(_lib.ptr(z[i]), B * 3 * H * W, seed, sid0 + i, _lib.stream_ptr(DEV)), "fill")
        else:
            _lib.check(lib.sinddm_normal_fill_samples(_lib.ptr(z[i]), B, 3 * H * W, _lib.ptr(sd), sid0 + i,
                                                      _lib.stream_ptr(DEV)), "fill_samples")
    torch.cuda.synchronize()
    return z


def _q_sample(d, y, yp, s, t, z):
    """sinddm_q_sample(x0 = y_prev (y at scale 0), x_orig = y, noise = z) at the host level t."""
    yd = y.to(DEV)
    if s == 0:
        return d._q_sample_impl(yd, None, t, z)
    return d._q_sample_impl(yp.to(DEV), None, t, z, x_orig=yd, gamma_row=d.gammas[s - 1].contiguous())


def _composed(net, d, y, yp, s, t_list, z, weight=None):
    """The yardstick: the route a user could write before the score call existed -- q_sample, the inference forward, torch ops
    -- on the same draws.  (map, level) in fp32 on the CPU."""
    B, _, H, W = y.shape
    w = torch.ones(H, W, device=DEV) if weight is None else weight.to(DEV)
    smap = torch.zeros(B, H, W, device=DEV)
    level = torch.zeros(len(t_list), B, device=DEV)
    for i, t in enumerate(t_list):
        eps = net.infer(_q_sample(d, y, yp, s, t, z[i]), None, t, float(s))
        m = w * (z[i] - eps).abs().sum(dim=1)
        smap += m
        level[i] = m.sum(dim=(1, 2))
    return smap.cpu(), level.cpu()


def _against_f64(golden, dim, y, yp, s, t_list, seeds=None, weight=None, tag=""):
    """Test 2's comparison for one call: returns (err_new_map, E_c_map, err_new_level, E_c_level, outputs of the call)."""
    net, d, sd, sched = _model(golden, dim)
    B, _, H, W = y.shape
    out = _call(net, d, y, yp, s, t_list, seeds=seeds, weight=weight)
    z = _draws(B, H, W, len(t_list), seeds=seeds)
    ref_map, ref_lev = score_f64(sched, sd, y, yp if s > 0 else None, s, t_list, z.cpu(), weight=weight)
    c_map, c_lev = _composed(net, d, y, yp, s, t_list, z, weight=weight)
    e_map, E_map = float((out[2].double() - ref_map).abs().max()), float((c_map.double() - ref_map).abs().max())
    e_lev, E_lev = float((out[3].double() - ref_lev).abs().max()), float((c_lev.double() - ref_lev).abs().max())
    print(f"[score {tag} dim {dim} B {B} {H}x{W} s {s}] map: new {e_map:.3e}  composed E_c {E_map:.3e}  (max |map| "
          f"{float(ref_map.abs().max()):.3e});  level: new {e_lev:.3e}  composed E_c {E_lev:.3e}  (max level "
          f"{float(ref_lev.abs().max()):.3e})")
    return e_map, E_map, e_lev, E_lev, out


def test_shapes_take_their_routes():
    from sinddm_amd import _lib
    lib = _lib.load()
    got = [plan(lib, dim, 0, B, H, W, ncu=0) for dim, B, H, W in SHAPES]
    assert [(p["fuse_tail"], p["last_fused"], p["gx_fused"]) for p in got[:2]] == [(1, 1, 1), (1, 0, 1)]
    assert got[1]["padded"] == 1 and got[1]["Wp"] == 20
    assert got[2]["fuse_tail"] == 0 and got[2]["padded"] == 0
    assert (got[3]["fuse_tail"], got[3]["last_fused"], got[3]["gx_fused"]) == (1, 1, 3)
    # three different endings: the plain fused kernel, the pitch kernel, the rows kernel
    assert len({(p["fuse_tail"], p["last_fused"] if p["fuse_tail"] else -1) for p in got}) == 3


# ---- 1: the draws and x_t ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,B,H,W", SHAPES, ids=IDS)
def test_x_t_is_q_sample_of_the_last_draw(golden, dim, B, H, W):
    net, d, _, _ = _model(golden, dim)
    y, yp = _pics(B, H, W)
    levels = [7, 55, 31]
    for s in (0, 2):
        assert s == 0 or 0.0 < float(d.gammas[s - 1][31]) < 1.0
        for seeds in (None, [11 + 5 * b for b in range(B)]):
            for n in (1, 2, 3):
                _, xt, _, _ = _call(net, d, y, yp, s, levels[:n], seeds=seeds)
                z = _draws(B, H, W, n, seeds=seeds)
                want = _q_sample(d, y, yp, s, levels[n - 1], z[n - 1]).cpu()
                assert torch.equal(xt, want), (s, seeds is not None, n)


# ---- 2: the map and the table against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,B,H,W", SHAPES, ids=IDS)
def test_map_and_table_against_float64(golden, dim, B, H, W):
    """err(new) <= 2 E_c, E_c the composed route's max-abs error against float64 on the same draws.  The factor covers the fused
    head's summation order and the fp32 running sum over the evaluations (tests/test_gpu_head.py: the fused and the unfused head
    already differ by kernel-path rounding).  Measured values: profiles/NOTES_r38.md."""
    y, yp = _pics(B, H, W)
    for s, seeds in ((2, [3 + b for b in range(B)]), (0, None)):
        e_map, E_map, e_lev, E_lev, _ = _against_f64(golden, dim, y, yp, s, [3, 36, 69, 99], seeds=seeds, tag="t2")
        assert E_map > 0 and E_lev > 0
        assert e_map <= 2 * E_map, (s, e_map, E_map)
        assert e_lev <= 2 * E_lev, (s, e_lev, E_lev)


# ---- 3: the level sums -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,B,H,W", SHAPES, ids=IDS)
def test_level_sums(golden, dim, B, H, W):
    """With one evaluation the map holds exactly the fp32 values the level sum adds: level_out[0, b] is within 1e-6 relative of
    their float64 sum (the contract of sinddm_l1_loss_rect_fwd_bwd).  A second call gives the same bits, in every output."""
    net, d, _, _ = _model(golden, dim)
    y, yp = _pics(B, H, W)
    w = torch.ones(H, W)
    w[::3, 1::2] = 0.25
    w[:2] = 0
    for s, weight, t in ((0, None, 12), (2, w, 88)):
        a = _call(net, d, y, yp, s, [t], weight=weight)
        want = level_sum_f64(a[2].numpy())
        got = a[3][0].double().numpy()
        rel = np.abs(got - want) / want
        print(f"[score t3 dim {dim} {H}x{W} s {s}] level sum rel err {rel.max():.3e}")
        assert rel.max() <= 1e-6, (s, rel)
    for s, weight in ((0, None), (2, w)):
        a = _call(net, d, y, yp, s, [5, 50, 95, 20], weight=weight)
        b = _call(net, d, y, yp, s, [5, 50, 95, 20], weight=weight)
        for u, v in zip(a[1:], b[1:]):
            assert torch.equal(u, v)
        # the evaluations' levels add up to the map (fp32 running sum against the sum of rounded level sums: loose)
        assert np.allclose(a[3].double().sum(dim=0).numpy(), level_sum_f64(a[2].numpy()), rtol=1e-5)


# ---- 4: the weight plane ---------------------------------------------------------------------------------------------------------
def test_weight_plane_zeros(golden):
    """dim 16, 40x52.  The weight is non-zero on the columns >= 40 only.  Zero-weight pixels are exactly 0 in the map and absent
    from the level sums; and a change of y by 1e3 confined to the columns <= 15 -- 24 pixels and more from any non-zero weight,
    past the network's reach of 16 -- changes no bit of the map, the level sums or x_t outside the changed columns."""
    dim, B, H, W = SHAPES[3]
    net, d, _, _ = _model(golden, dim)
    y, yp = _pics(B, H, W)
    w = torch.zeros(H, W)
    w[:, 40:] = hash_randn((H, 12), 5).abs() + 0.1
    levels = [90, 60, 10]
    for s in (0, 2):
        assert s == 0 or float(d.gammas[s - 1][10]) < 1.0
        a = _call(net, d, y, yp, s, levels, weight=w)
        full = _call(net, d, y, yp, s, levels)
        assert float(a[2][:, :, :40].abs().max()) == 0.0 and bool((a[2][:, :, 40:] > 0).all())
        assert bool((full[2] > 0).all())
        assert np.allclose(a[3].double().sum(dim=0).numpy(), level_sum_f64(a[2].numpy()), rtol=1e-5)
        y2 = y.clone()
        y2[:, :, :, :16] += 1e3
        b = _call(net, d, y2, yp, s, levels, weight=w)
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        # (the change did reach the call: x_t of the last level, 10, where gamma < 1 lets y through at scale 2 as well)
        assert torch.equal(a[1][:, :, :, 16:], b[1][:, :, :, 16:]) and not torch.equal(a[1], b[1])


# ---- 5: per-sample seeds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,H,W", [(16, 12, 16), (16, 13, 17), (20, 13, 17)], ids=IDS[:3])
def test_seeded_sample_does_not_depend_on_its_batch(golden, dim, H, W):
    net, d, _, _ = _model(golden, dim)
    y3, yp3 = _pics(3, H, W)
    levels = [8, 47, 93]
    for pos in (0, 2):
        y1, yp1 = y3[pos:pos + 1].clone(), yp3[pos:pos + 1].clone()
        seeds3 = [1000, 2000, 3000]
        seeds3[pos] = 424242
        for s in (0, 2):
            e1, E1, _, _, one = _against_f64(golden, dim, y1, yp1, s, levels, seeds=[424242], tag="t5 B1")
            e3, E3, _, _, three = _against_f64(golden, dim, y3, yp3, s, levels, seeds=seeds3, tag="t5 B3")
            assert torch.equal(one[1][0], three[1][pos])                          # x_t: bit-equal
            assert e1 <= 2 * E1 and e3 <= 2 * E3                                  # each map within test 2's tolerance


# ---- 6: it is the training loss ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,B,H,W", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_level_sums_are_the_training_loss(golden, dim, B, H, W):
    """level_out[i, :].sum() / (B 3 HW) against p_losses(t = t_i, noise = z_i) ('l1', the TRAINING forward).  With L the float64
    value, test 2 bounds |new - L| by 2 E_c and p_losses is E_p = |p_losses - L| away from it: |new - p_losses| <= 2 E_c + E_p."""
    net, d, sd, sched = _model(golden, dim)
    y, yp = _pics(B, H, W)
    levels = [4, 52, 97]
    norm = B * 3 * H * W
    for s in (0, 2):
        e_map, E_map, e_lev, E_lev, out = _against_f64(golden, dim, y, yp, s, levels, tag="t6")
        z = _draws(B, H, W, len(levels))
        ref = score_f64(sched, sd, y, yp if s > 0 else None, s, levels, z.cpu())[1].sum(dim=1) / norm
        for i, t in enumerate(levels):
            tt = torch.full((B,), t, device=DEV, dtype=torch.long)
            kw = dict(x_orig=y.to(DEV)) if s > 0 else {}
            with torch.no_grad():
                p = float(d.p_losses((yp if s > 0 else y).to(DEV), tt, s, noise=z[i], **kw))
            new = float(out[3][i].double().sum()) / norm
            E_p = abs(p - float(ref[i]))
            print(f"[score t6 dim {dim} s {s} t {t}] new {new:.8g}  p_losses {p:.8g}  float64 {float(ref[i]):.8g}")
            assert abs(new - p) <= 2 * B * E_lev / norm + E_p + 1e-7 * abs(p), (s, t, new, p)


# ---- 7: it sees what it should ----------------------------------------------------------------------------------------------------
def test_pasted_patch(golden):
    """dim 16 (he_state_dict(16): untrained He-normal weights), 40x52, scale 0, 4 levels x 2 draws through denoise_score with
    seeds.  The picture is a crop of the C1 training image (tests/golden/c1_pyramid.npz, scale_0) with a 3x3 gray patch pasted
    in (rows 20 ... 22, columns 30 ... 32; dilated by 16: rows 4 ... 38, columns 14 ... 48, 59 % of the plane).
    First half, as the issue words it: the arg-max of the pasted picture's map lies inside the patch dilated by 16 px --
    asserted.  Measured on the MI355X: the arg-max is (8, 32), inside.  It is ALSO the arg-max of the clean crop's map, scored
    under the same draws: the untrained net's largest score is where it was before the paste, so the assertion holds here
    without the patch being what it points at.
    Beside it, the property the construction does give, bit for bit: under the very draws the clean crop is scored under, the
    two maps differ only inside the dilated patch (the receptive radius), and the largest change lies there ((23, 30), +2.41).
    Second half -- the patch's mean score exceeds the image mean -- is NOT asserted: the synthetic net does not separate them
    (patch mean / image mean = 0.955).  The figures are printed; no detection claim is made (profiles/NOTES_r38.md)."""
    net, d, _, _ = _model(golden, 16)
    H, W = 40, 52
    pyr = golden("c1_pyramid.npz")
    crop = torch.from_numpy(pyr["scale_0"][4:4 + H, 6:6 + W].transpose(2, 0, 1).copy()).float().div(255).mul(2).sub(1)
    pic = crop.clone()
    pic[:, 20:23, 30:33] = 0.0
    patch = torch.zeros(H, W, dtype=torch.bool)
    patch[20:23, 30:33] = True
    near = dilate(patch, 16)
    assert 0 < int(near.sum()) < H * W and float((pic - crop).abs().max()) > 0.1
    batch = torch.stack([crop, pic]).to(DEV)
    seeds = [21, 22, 21, 22]                                                        # both rows under the same two draws
    smap, table = d.denoise_score(batch, 0, levels=[5, 35, 65, 95], draws=2, seeds=seeds)
    torch.cuda.synchronize()
    smap = smap.cpu()
    excess = smap[1] - smap[0]
    assert float(excess[~near].abs().max()) == 0.0                                 # the reach of the network, bit for bit
    ey, ex = divmod(int(excess.abs().argmax()), W)
    assert bool(near[ey, ex]) and float(excess.abs().max()) > 0
    iy, ix = divmod(int(smap[1].argmax()), W)                                      # the issue's first half, as it words it
    cy, cx = divmod(int(smap[0].argmax()), W)
    ratio = float(smap[1][patch].mean() / smap[1].mean())
    print(f"[score t7] arg-max of the pasted picture's map {(iy, ix)} (inside the dilated patch: {bool(near[iy, ix])}; of the "
          f"clean crop's map: {(cy, cx)}); patch mean / image mean = {ratio:.4f}; excess max {float(excess.max()):.4f} at "
          f"{(ey, ex)}")
    assert bool(near[iy, ix]), (iy, ix)
    assert np.isfinite(ratio)


# ---- 8: error codes -----------------------------------------------------------------------------------------------------------------
def test_error_codes_come_before_any_device_work(golden):
    from sinddm_amd import _lib
    from sinddm_amd.models import _workspace
    lib = _lib.load()
    dim, B, H, W = SHAPES[0]
    net, d, _, _ = _model(golden, dim)
    y, yp = (v.to(DEV) for v in _pics(B, H, W))
    n = 3
    need = lib.sinddm_score_workspace_bytes(dim, B, H, W, n)
    ws = _workspace(DEV, need)
    gx, xt, g = _guarded((B, 3, H, W))
    gm, smap, _ = _guarded((B, H, W))
    gl, lev, _ = _guarded((n, B))
    wgt = torch.ones(H * W + 4, device=DEV)
    sds = torch.zeros(2 * B + 1, dtype=torch.int32, device=DEV)
    gamma = d.gammas[1].contiguous()
    tl = (C.c_int * n)(3, 40, 80)
    neg = (C.c_int * n)(3, -1, 80)
    good = dict(params=_lib.ptr(net.flat_params), packed=_lib.ptr(net.packed_weights()), y=_lib.ptr(y), y_prev=_lib.ptr(yp),
                x_t=xt.data_ptr(), ta=_lib.ptr(d.sqrt_alphas_cumprod), tb=_lib.ptr(d.sqrt_one_minus_alphas_cumprod),
                gamma=_lib.ptr(gamma), t_list=tl, n=n, map=smap.data_ptr(), lev=lev.data_ptr(), dim=dim, B=B, H=H, W=W,
                ws=ws.data_ptr(), ws_bytes=need, weight=None, seeds=None)

    def call(**kw):
        a = dict(good, **kw)
        opts = _lib.ScoreOpts(a["weight"], a["seeds"])
        rc = lib.sinddm_score_chain(a["params"], a["packed"], a["y"], a["y_prev"], a["x_t"], a["ta"], a["tb"], a["gamma"],
                                    a["t_list"], a["n"], 2.0, 5, SID0, a["map"], a["lev"], a["dim"], a["B"], a["H"], a["W"],
                                    a["ws"], a["ws_bytes"], _lib.stream_ptr(DEV), C.byref(opts))
        torch.cuda.synchronize()
        return rc

    BADARG, BADSHAPE, WORKSPACE = -1, -2, -3
    cases = [(dict(params=None), BADARG), (dict(packed=None), BADARG), (dict(y=None), BADARG), (dict(x_t=None), BADARG),
             (dict(ta=None), BADARG), (dict(tb=None), BADARG), (dict(t_list=None), BADARG), (dict(map=None), BADARG),
             (dict(lev=None), BADARG), (dict(ws=None), BADARG),
             (dict(y_prev=None), BADARG), (dict(gamma=None), BADARG),                     # one of the pair without the other
             (dict(n=0), BADARG), (dict(n=1025), BADARG), (dict(t_list=neg), BADARG),
             (dict(B=0), BADARG), (dict(H=0), BADARG), (dict(W=-3), BADARG),
             (dict(weight=wgt.data_ptr() + 4), BADARG), (dict(seeds=sds.data_ptr() + 4), BADARG),
             (dict(y=_lib.ptr(y) + 4), BADARG), (dict(x_t=xt.data_ptr() + 4), BADARG), (dict(map=smap.data_ptr() + 4), BADARG),
             (dict(dim=3), BADSHAPE), (dict(B=65536), BADSHAPE), (dict(H=30000, W=30000), BADSHAPE),
             (dict(ws_bytes=need - 1), WORKSPACE), (dict(ws_bytes=0), WORKSPACE)]
    for kw, want in cases:
        assert call(**kw) == want, kw
        for big in (gx, gm, gl):
            assert bool(big.isnan().all()), kw                                            # nothing was written
    assert call() == 0                                                                    # and the good call runs
    assert not bool(xt.isnan().any()) and not bool(smap.isnan().any()) and not bool(lev.isnan().any())
    assert bool(gx[:g].isnan().all()) and bool(gm[-g:].isnan().all()) and bool(gl[-g:].isnan().all())


# ---- 9: the Python layers are this call ---------------------------------------------------------------------------------------------
def test_denoise_score_is_the_chain_call(golden):
    """draws folded into the batch (row b * draws + r), the map the mean over levels, draws and channels times the weight, the
    table the level means over sum(w): recomputed here from one direct call with the same seeds."""
    from sinddm_amd.score import score_stream_id
    dim, B, H, W = SHAPES[1]
    net, d, _, _ = _model(golden, dim)
    y, yp = _pics(B, H, W)
    w = torch.ones(H, W)
    w[3:6, 2:9] = 0
    levels, draws = [2, 40, 77, 99, 60], 2
    seeds = [100 + r for r in range(B * draws)]
    smap, table = d.denoise_score(y.to(DEV), 2, y_prev=yp.to(DEV), levels=levels, draws=draws, seeds=seeds, weight=w.to(DEV))
    torch.cuda.synchronize()
    rep = lambda t: t.repeat_interleave(draws, dim=0)
    _, _, m, lev = _call(net, d, rep(y), rep(yp), 2, levels, sid0=score_stream_id(2, 0), seeds=seeds, weight=w)
    assert tuple(smap.shape) == (B, H, W) and tuple(table.shape) == (len(levels), B)
    want_map = m.view(B, draws, H, W).mean(dim=1) / (3.0 * len(levels))
    want_tab = lev.view(len(levels), B, draws).mean(dim=2) / (3.0 * float(w.double().sum()))
    # (1e-6: the device divides by a scalar through its reciprocal)
    assert torch.allclose(smap.cpu(), want_map, rtol=1e-6, atol=0) and torch.allclose(table.cpu(), want_tab, rtol=1e-6, atol=0)
    assert float(smap.cpu()[:, 3:6, 2:9].abs().max()) == 0.0
    # unseeded: a key from torch's generator; reproducible under manual_seed, different draws otherwise
    torch.manual_seed(3)
    a = d.denoise_score(y.to(DEV), 0, levels=[10, 90])[0].cpu()
    torch.manual_seed(3)
    b = d.denoise_score(y.to(DEV), 0, levels=[10, 90])[0].cpu()
    c = d.denoise_score(y.to(DEV), 0, levels=[10, 90])[0].cpu()
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_trainer_score_writes_its_report(golden, tmp_path):
    """MultiscaleTrainer.score over the C1 pyramid (closed-form weights, dim 32, T = 20): the training pyramid alone, then a
    picture side by side; the report, the PNGs, and an edit map that `--mode edit --edit_map` reads without conversion."""
    import json
    from PIL import Image
    from test_gpu_chain_guided import _trainer
    tr, meta = _trainer(golden, tmp_path)
    n = meta["n_scales"]
    res = str(tmp_path / "res")
    report, maps = tr.score(levels=3, draws=2, seeds=[5, 6])
    assert [r["scale"] for r in report["scales"]] == list(range(n)) and sorted(maps) == list(range(n))
    for s, r in enumerate(report["scales"]):
        h, w = tr.ema_model.image_sizes[s]
        assert tuple(maps[s].shape) == (1, h, w) and r["levels"] == [0, 10, 19]
        assert len(r["table"]) == 1 and len(r["table"][0]) == 3 and all(np.isfinite(v) and v > 0 for v in r["table"][0])
    assert json.load(open(os.path.join(res, "score_report.json"))) == report
    assert not os.path.exists(os.path.join(res, "score_edit_map.png"))
    h, w = tr.ema_model.image_sizes[n - 1]
    pic = tr.data_list[n - 1][0][0].cpu().clone()
    pic[:, 40:50, 60:75] = 0.0
    report2, maps2 = tr.score(image=pic, levels=3, draws=2, scales=(1, n - 1), seeds=[5, 6])
    assert [r["scale"] for r in report2["scales"]] == list(range(1, n))
    assert tuple(maps2[n - 1].shape) == (2, h, w)
    # row 0: the training image, under the same draws (to rounding: the convolutions' route may change with the batch)
    assert torch.allclose(maps2[n - 1][0], maps[n - 1][0], rtol=1e-3, atol=1e-5)
    e = Image.open(os.path.join(res, "score_edit_map.png"))
    assert e.mode == "L" and e.size == (w, h)
    back = torch.from_numpy(np.asarray(e.convert("L").resize((w, h), Image.BILINEAR), dtype=np.float32).copy()).div(255)
    assert float(back.min()) >= 0.0 and float(back.max()) <= 1.0
    for s in range(1, n):
        assert os.path.exists(os.path.join(res, f"score_s{s}.png"))
    # the edit mode takes the file as its strength map
    frames = tr.edit(back, batch_size=1, save_images=False, seeds=[9])
    assert tuple(frames[-1].shape) == (1, 3, h, w)
    tr.ema_model.tile = (False, True)
    with pytest.raises(NotImplementedError):
        tr.score(levels=2, draws=1)


def test_trainer_score_under_a_train_mask(golden, tmp_path):
    """MultiscaleTrainer(train_mask=...).score: the hard mask of every scale is the weight plane -- the holes are exact zeros in
    every row's map, the table is the mean over the valid pixels (recomputed here from the map), and the edit map is normalised
    over the valid pixels only (score.score_edit_map(valid=...)): a hole comes out 0."""
    from PIL import Image
    from sinddm_amd.score import score_edit_map
    from test_gpu_chain_guided import _trainer
    meta = golden("g11_img_scales.json")["C1"]
    w, h = meta["sizes"][-1]
    valid = torch.ones(h, w)
    valid[30:60, 20:70] = 0
    tr, meta = _trainer(golden, tmp_path, train_mask=valid)
    n = meta["n_scales"]
    assert tr.train_mask_hard is not None
    pic = tr.data_list[n - 1][0][0].cpu().clone()
    pic[:, 70:80, 90:110] = 0.0
    report, maps = tr.score(image=pic, levels=[0, 10, 19], draws=2, seeds=[5, 6])
    for s in range(n):
        hard = tr.train_mask_hard[s] > 0
        assert 0 < int(hard.sum()) < hard.numel()
        m = maps[s]
        assert float(m[:, ~hard].abs().max()) == 0.0 and bool((m[:, hard] > 0).all())
        table = torch.tensor(report["scales"][s]["table"], dtype=torch.float64)      # [row][level]
        want = m.double().sum(dim=(1, 2)).cpu() / float(hard.sum())                # mean over levels of the level means
        assert torch.allclose(table.mean(dim=1), want, rtol=1e-5, atol=0)
    res = str(tmp_path / "res")
    e = torch.from_numpy(np.asarray(Image.open(os.path.join(res, "score_edit_map.png")), dtype=np.float32).copy()).div(255)
    hard = (tr.train_mask_hard[n - 1] > 0).cpu()
    want = score_edit_map(maps[n - 1][1].cpu(), maps[n - 1][0].cpu(), valid=hard)
    assert float(e[~hard].abs().max()) == 0.0 and float((e - want).abs().max()) <= 0.5 / 255 + 1e-6
    assert float(e.max()) > 0.0
