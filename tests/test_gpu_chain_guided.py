"""The fused sampler chain with options (sinddm_sample_chain_ex): ROI edit maps and caller-supplied noise inside the three
tail kernels of a chain step (final conv + reverse step on plain rows, on padded rows, and the unfused reverse step).

  * ROI-guided sampling takes one chain call per scale and still matches the oracle (replay of the logged draws);
  * the fused edit equals the step-by-step edit (sinddm_reverse_step_edit) on every tail kernel, same numbers in;
  * a noise buffer filled with the in-kernel stream's own numbers reproduces the Philox run bit for bit (this pins the
    whole-batch indexing of two-stream runs and the unaligned reads of the padded-row kernel);
  * `chain_noise = True` equals the step-by-step route over a whole scale.
reference SinDDM/models.py:291-298,430-431 (ROI edit), 449-459 (p_sample), 501-547 (the loop)
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import max_abs, rel_l2
from oracle import sinddm_oracle as O
from sinddm_amd.configs import build_diffusion
from sinddm_amd.synth import closed_form_state_dict, hash_randn, noise_key

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

BBS, TARGET = [[20, 30, 40, 36], [35, 50, 30, 30]], [10, 12, 30, 40]       # the boxes of test_gpu_e2e's ROI test


def _fill(n, seed, stream):
    from sinddm_amd import _lib
    lib = _lib.load()
    out = torch.empty(n, device=DEV)
    _lib.check(lib.sinddm_normal_fill(_lib.ptr(out), n, seed, stream, _lib.stream_ptr(DEV)), "sinddm_normal_fill")
    return out


def _trainer(golden, tmp_path, dim=32, T=20, batch=2, **kw):                # the C1 recipe of tests/test_gpu_e2e.py
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
                           results_folder=str(tmp_path / "res"), device=DEV, **kw)
    return tr, meta


def _roi_patches(golden, meta, target_roi):
    pyr = golden("c1_pyramid.npz")
    n, sf = meta["n_scales"], meta["scale_factor"]
    out = []
    for s in range(n):
        ten = torch.from_numpy(pyr[f"scale_{s}"].transpose(2, 0, 1).copy()).float().div(255).mul(2).sub(1)[None]
        y, x, h, w = [int(b / np.power(sf, n - s - 1)) for b in target_roi]
        out.append(ten[:, :, y:y + h, x:x + w])
    return out


# ---- 1, 2: the public ROI mode ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def roi_run(golden, tmp_path_factory):
    """MultiscaleTrainer.roi_guided_sampling on the C1 pyramid (dim 32, T = 20, B = 2) with NO injected noise; the draws it
    consumed are logged."""
    tr, meta = _trainer(golden, tmp_path_factory.mktemp("roi_chain"))
    d = tr.ema_model
    d.draw_log = []
    torch.manual_seed(4321)
    outs = tr.roi_guided_sampling(custom_t_list=d.num_timesteps_ideal[1:], target_roi=TARGET, roi_bb_list=BBS,
                                  save_unbatched=False, batch_size=2, scale_mul=(1, 1), save_images=False)
    log, d.draw_log = d.draw_log, None
    assert d.roi_guided_sampling is False
    return dict(outs=outs, log=log, meta=meta, ideal=list(d.num_timesteps_ideal))


def test_roi_run_takes_the_chain(roi_run):
    """One chain call per scale, guided scales included (they used to log one 'step' draw per reverse step)."""
    assert [e[0] for e in roi_run["log"]] == ["init", "chain", "renoise", "chain", "renoise", "chain"]


def test_roi_chain_replayed_through_oracle(roi_run, golden):
    """The draws of the run above, regenerated with sinddm_normal_fill and replayed through the oracle's ROI chain:
    <= 1e-4 rel-L2 per scale; and the guided result is far (> 1e-2) from the oracle's unguided chain on the same draws."""
    from sinddm_amd import _lib
    lib = _lib.load()
    meta, log, B = roi_run["meta"], roi_run["log"], 2
    sizes = [tuple(s) for s in meta["image_sizes_hw"]]
    noises = {}
    for e in log:
        if e[0] == "init":
            noises[("init", 0)] = e[3].cpu()
        elif e[0] == "renoise":
            noises[("renoise", e[1])] = e[3].cpu()
        else:
            assert e[0] == "chain", e[0]
            _, s, seed, ts = e
            numel = B * 3 * sizes[s][0] * sizes[s][1]
            for i, t in enumerate(ts):
                z = torch.empty(numel, device=DEV)
                _lib.check(lib.sinddm_normal_fill(_lib.ptr(z), numel, seed, i, _lib.stream_ptr(DEV)), "normal_fill")
                noises[("step", s, t)] = z.view(B, 3, *sizes[s]).cpu()
    assert sum(1 for k in noises if k[0] == "step") == sum(roi_run["ideal"])
    sched = O.make_schedule(20, meta["n_scales"], meta["rescale_losses"], 1, train_full_t=True)
    roi = dict(bbs=BBS, target_patch=_roi_patches(golden, meta, TARGET), scale_factor=meta["scale_factor"])
    with torch.no_grad():
        ref = O.sample_chain(sched, closed_form_state_dict(32), sizes, noises, B, roi=roi)
        plain = O.sample_chain(sched, closed_form_state_dict(32), sizes, noises, B)
    errs = [rel_l2(a.cpu(), b) for a, b in zip(roi_run["outs"], ref)]
    far = [rel_l2(a.cpu(), b) for a, b in zip(roi_run["outs"], plain)]
    print("ROI chain vs oracle replay, rel-L2 per scale:", ["%.2e" % e for e in errs], "to the unguided chain:",
          ["%.2e" % e for e in far])
    assert max(errs) <= 1e-4, errs
    assert far[0] > 1e-2, far                              # the edit is not a no-op


# ---- 3, 4, 6: the library call on every tail kernel ----------------------------------------------------------------------
# (cfg, dim, s, B, two streams, steps).  Which tail a shape takes (sinddm_fwd.hip: fuse_tail / plan_pads_rows / fwd_pitch):
#   H*W % 4 == 0                      -> final_conv_reverse_step_kernel                   (dim 160, 48x64)
#   W % 4 != 0 and the plan pads rows -> final_conv_reverse_step_pitch_kernel            (dim 160: 67x90, 133x177)
#   H*W % 4 != 0, plain rows          -> final_conv1x1 + reverse_step_rows_kernel: the plan pads rows only when every
#                                        block's channel count is a multiple of 4; dim 20 has dim/2 = 10 -> plain rows
SHAPES = [("C2", 160, 0, 16, False, [700, 2, 0]),
          ("C2", 160, 1, 16, True, [400, 1, 0]),
          ("C2", 160, 3, 4, False, [311, 2, 0]),
          ("C2", 20, 3, 4, False, [311, 2, 0])]
IDS = ["plain_48x64", "pitch_67x90_two_streams", "pitch_133x177", "unfused_dim20_133x177"]


def _rows_padded(lib, dim, B, H, W):
    """Padded rows cost a padded copy of the input on top of activations of the rounded-up width, so the workspace of
    width W is LARGER than that of the next multiple of 4; with plain rows it is smaller."""
    Wr = (W + 3) // 4 * 4
    return W % 4 != 0 and lib.sinddm_workspace_bytes(dim, B, H, W) > lib.sinddm_workspace_bytes(dim, B, H, Wr)


def _setup(cfg, dim, s, B):
    """Diffusion + inputs + ROI state of one shape.  Boxes are given in pixels OF THE SCALE and converted to the full-size
    coordinates `roi_edit_maps` takes: two overlapping ones (the second starts at x = 13, not a multiple of 4) and one that
    touches the right and the bottom edge."""
    net, d = build_diffusion(cfg, dim=dim, device=DEV)
    H, W = d.image_sizes[s]
    f = float(np.power(d.scale_factor, d.n_scales - s - 1))
    assert f > 1.3                                              # (a guided scale; makes the conversion below exact)
    boxes = [[5, 8, 20, 24], [14, 13, 17, 30], [H - 11, W - 9, 11, 9]]          # [y, x, h, w]
    d.roi_bbs = [[int(math.ceil(v * f + 1e-6)) for v in bb] for bb in boxes]
    assert [[int(v / f) for v in bb] for bb in d.roi_bbs] == boxes
    d.roi_target_patch = [(hash_randn((1, 3, 9, 7), 90 + i) * 0.6).clamp(-1, 1).to(DEV) for i in range(d.n_scales)]
    ew, ec = d.roi_edit_maps(s, H, W, DEV)
    assert float(ew[4, 8]) == 1.0 and abs(float(ew[5, 8]) - 0.2) < 1e-6 and abs(float(ew[14, 13]) - 0.04) < 1e-6
    assert float(ew[14, 12]) != float(ew[14, 13]) and abs(float(ew[H - 1, W - 1]) - 0.2) < 1e-6
    x0 = (hash_randn((B, 3, H, W), 31 + s) * 0.8).to(DEV)
    xt = (hash_randn((B, 3, H, W), 32 + s) * 0.5).clamp(-1, 1).to(DEV)
    d.img_prev_upsample = xt
    return net, d, H, W, x0, xt, ew, ec


def _chain_ex(net, d, s, x0, xt, ts, seed, sid0, dim, aux=False, edit=None, noise=None, opts_null=False, entry="ex"):
    from sinddm_amd import _lib
    from sinddm_amd.models import _aux_stream, _workspace
    lib = _lib.load()
    B, _, H, W = x0.shape
    n = len(ts)
    xa, xb, eps = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
    tab = d._coef_table(s)
    coefs = (_lib.StepCoefs * max(n, 1))(*[tab[t] for t in ts])
    tl = (C.c_int * max(n, 1))(*ts)
    ws = _workspace(DEV, lib.sinddm_workspace_bytes(dim, B, H, W))
    flag = C.c_int(-1)
    opts = _lib.ChainOpts()
    if edit is not None:
        opts.edit_w, opts.edit_c = (_lib.ptr(e) if e is not None else None for e in edit)
    opts.noise = _lib.ptr(noise)
    args = [_lib.ptr(net.flat_params), _lib.ptr(net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
            coefs, tl, n, float(s), seed, sid0, dim, B, H, W, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
            _aux_stream(DEV) if aux else None, C.byref(flag)]
    if entry == "ex":
        rc = lib.sinddm_sample_chain_ex(*args, None if opts_null else C.byref(opts))
    else:
        rc = lib.sinddm_sample_chain2(*args)
    torch.cuda.synchronize()
    return rc, flag.value, (xb if flag.value == 1 else xa)


def _draws(x0, n_steps, seed, sid0):
    """The numbers the in-kernel stream gives steps 0..n-1 of a run, as the step-major buffer the chain call takes."""
    return torch.stack([_fill(x0.numel(), seed, sid0 + i).view_as(x0) for i in range(n_steps)]).contiguous()


@pytest.mark.parametrize("cfg,dim,s,B,aux,ts", SHAPES, ids=IDS)
def test_fused_edit_equals_stepwise_edit(cfg, dim, s, B, aux, ts):
    """sinddm_sample_chain_ex with edit maps == _p_sample_host_t with roi_guided_sampling (sinddm_net_forward +
    sinddm_reverse_step_edit per step) fed the chain's own draws; three steps incl. t = 0; the 3-step bound of
    test_gpu_sampler_shapes.  With a second stream the result equals the single-stream call bit for bit."""
    from sinddm_amd import _lib
    lib = _lib.load()
    net, d, H, W, x0, xt, ew, ec = _setup(cfg, dim, s, B)
    padded = _rows_padded(lib, dim, B, H, W)
    assert padded == (dim == 160 and W % 4 != 0)
    if dim == 20:
        assert (H * W) % 4 != 0 and not padded             # -> final_conv1x1 + reverse_step_rows_kernel
    seed = 515151 + s
    d.roi_guided_sampling = True
    x = x0.clone()
    for i, t in enumerate(ts):
        z = _fill(x.numel(), seed, i).view_as(x)
        d.noise_fn = lambda kind, shape, ss, tt, dev, z=z: z
        x = d._p_sample_host_t(x, t, s)
    d.noise_fn = None
    rc, flag, y = _chain_ex(net, d, s, x0, xt, ts, seed, 0, dim, aux=aux, edit=(ew, ec))
    assert rc == 0 and flag in (0, 1)
    assert torch.isfinite(y).all()
    err, bound = max_abs(y.cpu(), x.cpu()), 4e-6 * max(1.0, float(x.abs().max()))
    print(f"{cfg} dim {dim} s={s} {H}x{W} B={B}: fused edit vs stepwise edit max-abs {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # the edit is not a no-op: the unguided call lands elsewhere
    _, _, y_plain = _chain_ex(net, d, s, x0, xt, ts, seed, 0, dim, aux=aux)
    assert max_abs(y_plain.cpu(), y.cpu()) > 1e-2
    if aux:
        _, _, y1 = _chain_ex(net, d, s, x0, xt, ts, seed, 0, dim, aux=False, edit=(ew, ec))
        assert torch.equal(y, y1)
    # ... and the public route produces exactly this run
    torch.manual_seed(11)
    seed_api = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
    torch.manual_seed(11)
    d.two_streams = aux
    y_api = d._run_steps(x0.clone(), s, ts)
    _, _, y2 = _chain_ex(net, d, s, x0, xt, ts, seed_api, 0, dim, aux=aux, edit=(ew, ec))
    assert torch.equal(y_api, y2)


# B = 1: 3*133*177 % 4 == 3 -- the flat unfused kernel's last quad is partial, with recorded noise too
@pytest.mark.parametrize("with_edit", [False, True], ids=["plain", "edit"])
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts", SHAPES + [("C2", 20, 3, 1, False, [311, 2, 0])],
                         ids=IDS + ["unfused_dim20_133x177_B1_partial_quad"])
def test_noise_buffer_equals_philox(cfg, dim, s, B, aux, ts, with_edit):
    """`noise` = what sinddm_normal_fill gives for (seed, stream_id0 + i) reproduces the call without it, bit for bit."""
    net, d, H, W, x0, xt, ew, ec = _setup(cfg, dim, s, B)
    seed, sid0 = 777 + s, 5
    edit = (ew, ec) if with_edit else None
    rc0, _, y0 = _chain_ex(net, d, s, x0, xt, ts, seed, sid0, dim, aux=aux, edit=edit)
    rc1, _, y1 = _chain_ex(net, d, s, x0, xt, ts, 0, 0, dim, aux=aux, edit=edit, noise=_draws(x0, len(ts), seed, sid0))
    assert rc0 == 0 and rc1 == 0
    assert torch.equal(y0, y1)
    # the buffer is what is read: other numbers, another result
    _, _, y2 = _chain_ex(net, d, s, x0, xt, ts, 0, 0, dim, aux=aux, edit=edit, noise=_draws(x0, len(ts), seed + 1, sid0))
    assert not torch.equal(y0, y2)


def test_chain_ex_arguments():
    from sinddm_amd import _lib
    cfg, dim, s, B, aux, ts = SHAPES[1]
    net, d, H, W, x0, xt, ew, ec = _setup(cfg, dim, s, B)
    assert _chain_ex(net, d, s, x0, xt, ts, 1, 0, dim, edit=(ew, None))[0] == -1          # SINDDM_E_BADARG
    assert _chain_ex(net, d, s, x0, xt, ts, 1, 0, dim, edit=(None, ec))[0] == -1
    # opts = NULL (and opts with every member NULL) is sinddm_sample_chain2, bit for bit
    rc2, f2, y2 = _chain_ex(net, d, s, x0, xt, ts, 99, 3, dim, aux=aux, entry="chain2")
    rc0, f0, y0 = _chain_ex(net, d, s, x0, xt, ts, 99, 3, dim, aux=aux, opts_null=True)
    rc1, f1, y1 = _chain_ex(net, d, s, x0, xt, ts, 99, 3, dim, aux=aux)
    assert rc2 == rc0 == rc1 == 0 and f2 == f0 == f1
    assert torch.equal(y2, y0) and torch.equal(y2, y1)
    # an empty run with options: nothing happens, the result is where it was
    rc, flag, y = _chain_ex(net, d, s, x0, xt, [], 1, 0, dim, aux=aux, edit=(ew, ec), noise=_draws(x0, 1, 1, 0))
    assert rc == 0 and flag == 0 and torch.equal(y, x0)
    assert _lib.load().sinddm_abi_version() == 3


# ---- 5: chain_noise over a whole scale -----------------------------------------------------------------------------------
# Bound = 2 x the max-abs distance between the PLAIN sinddm_sample_chain and the step-by-step path over the same two whole-scale
# runs with identical draws, measured on the commit before this feature (see the docstring below): both were 0.
WHOLE_SCALE = [("C2", 1, 16, 521, 2 * 0.0),
               ("C3", 5, 4, 118, 2 * 0.0)]


@pytest.mark.parametrize("cfg,s,B,n_steps,bound", WHOLE_SCALE, ids=["C2_s1_B16_521", "C3_s5_B4_118"])
def test_chain_noise_equals_stepwise_over_a_whole_scale(cfg, s, B, n_steps, bound, monkeypatch):
    """The full default run of a scale (p_sample_via_scale_loop, custom_t = None) with a hash-keyed `noise_fn`, dim 160:
    `chain_noise = True` (the draws handed to sinddm_sample_chain_batch in >= 3 pieces) against the step-by-step route the
    fixtures pin.  This ties the fused tail kernels to the pinned path over a whole scale, not over three steps.

    The bound is measured, not chosen: on commit 331afdd (the parent of this feature), MI355X with 256 CUs, the plain
    sinddm_sample_chain and the step-by-step path (sinddm_net_forward + sinddm_reverse_step per step) fed identical draws
    (sinddm_normal_fill(seed, i)) ended, after all 521 steps of C2 scale 1 (67x90) at batch 16 and all 118 steps of C3's
    finest scale (411x512) at batch 4, at max-abs 0.0 / rel-L2 0.0: the fused tail accumulates the final conv and evaluates
    the step in the same order as the two separate kernels, and both routes launch the same convolution kernels on one box.
    Twice that figure is 0: the two routes must agree bit for bit (profiles/NOTES_r08.md).

    The draws come from the library's counter-based generator keyed on noise_key(kind, s, t) instead of synth.hash_randn:
    hash_randn takes 0.5 s of CPU per C3 step tensor here (about 60 s for that run alone, twice: once per route); batch and
    step counts are the ones asked for.  A hash-keyed generator does not see the order of the calls; the test compares the
    order itself."""
    from sinddm_amd import _lib, models
    lib = _lib.load()
    net, d = build_diffusion(cfg, dim=160, device=DEV)
    H, W = d.image_sizes[s]
    assert d.num_timesteps_ideal[s] - 1 == n_steps
    img = (hash_randn((B, 3, H, W), 32 + s) * 0.5).clamp(-1, 1).to(DEV)
    fetched = []

    def keyed(kind, shape, ss, tt, dev):
        fetched.append((kind, ss, tt))
        return _fill(int(np.prod(shape)), noise_key(kind, ss, tt), 0).view(shape)

    d.noise_fn = keyed
    ref = d.p_sample_via_scale_loop(B, img, s)                  # chain_noise = False: the pinned step-by-step route
    order_ref, fetched = fetched, []
    assert len(order_ref) == n_steps + 1
    per = (n_steps + 2) // 3                                    # steps per piece: three pieces
    monkeypatch.setattr(models, "CHAIN_NOISE_BYTES", per * B * 3 * H * W * 4)
    pieces = []
    real = lib.sinddm_sample_chain_batch
    monkeypatch.setattr(lib, "sinddm_sample_chain_batch", lambda *a: (pieces.append(a[8]), real(*a))[1])
    d.chain_noise = True
    got = d.p_sample_via_scale_loop(B, img, s)
    torch.cuda.synchronize()
    assert len(pieces) >= 3 and sum(pieces) == n_steps and max(pieces) == per, pieces
    assert fetched == order_ref                                 # same draws asked for, in the same order
    assert torch.isfinite(got).all()
    err = max_abs(got.cpu(), ref.cpu())
    print(f"{cfg} s={s} {H}x{W} B={B} {n_steps} steps in {len(pieces)} pieces: chain_noise vs stepwise max-abs {err:.3e} "
          f"rel-L2 {rel_l2(got.cpu(), ref.cpu()):.3e} (bound {bound})")
    assert err <= bound
