"""The host-side plan of one run of reverse steps at one scale: what `MultiScaleGaussianDiffusion._run_steps` and
`_p_sample_host_t` run.  Plain Python: no device work of its own, no library call.  `RunPlan` resolves the schedule, the maps,
the noise source and the halo ONCE and holds one `Step` record per reverse step; the chain route (`models._ChainCall`) packs
records into the arrays of a library call (`pack_steps`), the step-by-step route walks them through the single-step entries.
A new per-step scalar is derived in `RunPlan.__init__`, a new combination that is not built is a row of `NOT_BUILT`."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

from . import _lib
from .functions import gate_thresholds, keep_windows, layout_strengths, resample_schedule, stride_schedule

# The combinations of options that are not built, (option, the option it cannot go with) -> what NotImplementedError says.
NOT_BUILT = {
    ("keep_maps", "clip"): "keep_maps with clip_guided_sampling: the CLIP-guided step runs in eager torch ops and has no "
                           "known-region replacement",
    ("keep_gated", "clip"): "keep_gated with clip_guided_sampling: the CLIP-guided step runs in eager torch ops and has no "
                            "known-region replacement to gate",
    ("layout_maps", "clip"): "layout_maps with clip_guided_sampling: the CLIP-guided step runs in eager torch ops and has no "
                             "layout pull",
    ("resample", "clip"): "resample with clip_guided_sampling: the CLIP-guided step runs in eager torch ops and has no "
                          "resampling jump",
    ("few_step", "clip"): "sample_steps / solver_order / eta with clip_guided_sampling: the CLIP-guided step runs in eager "
                          "torch ops on the reference's own schedule",
    ("seed_mix", "clip"): "seed_mix with CLIP-guided sampling",
    ("few_step", "resample"): "sample_steps / solver_order / eta with resample: a resampling jump inside a strided or multistep "
                              "run is not built",
    ("layout_maps", "resample"): "layout_maps with resample: the layout pull inside a resampling jump is not built",
    ("layout_maps", "solver_order"): "solver_order = 2 with layout_maps: the multistep step through a layout pull is not built",
    ("strided_step", "clip_or_jump"): "a strided or multistep step under CLIP guidance or before a resampling jump",
    ("patch_refine", "keep_maps"): "patch_refine with keep_maps: a vote that respects the known region is not built "
                                   "(MultiscaleTrainer.refine takes a weight map)",
    ("patch_refine", "layout_maps"): "patch_refine with layout_maps: the vote between the scales of a layout-conditioned run "
                                     "is not built",
    ("patch_refine", "roi"): "patch_refine with ROI guidance: the vote between the scales of an ROI-guided run is not built",
    ("keep_window", "tile"): "keep_window with tile: a window across the wrapped border of a tiled run is not built",
    ("keep_window", "layout_maps"): "keep_window with layout_maps: the block means of the layout pull do not survive a crop",
    ("keep_window", "clip"): "keep_window with clip_guided_sampling: the CLIP-guided step runs in eager torch ops on the "
                             "whole image",
    ("keep_window", "noise_fn"): "keep_window with a caller's noise_fn: the windowed run draws by absolute position from "
                                 "per-sample seeds",
}
_ON = {"clip": lambda d: d.clip_guided_sampling, "resample": lambda d: d._resample_cfg() is not None}


def sampling_defaults() -> dict:
    """The sampling options: every attribute a run reads off the diffusion object, name -> the value that means "option off".
    A fresh dict with fresh mutable values per call.  `MultiScaleGaussianDiffusion.__init__` assigns exactly these, as plain
    attributes; `MultiScaleGaussianDiffusion.sampling(**options)` sets some of them for the length of a `with` block.  None
    of them is stored in checkpoints; the training options (`train_tile`, `train_weights`, `train_crop`, ...) are not here."""
    return {
        # tileable sampling: (wrap_y, wrap_x) -- on a wrapped axis the sample's borders wrap around, i.e. the network is
        # evaluated as if every convolution padded circularly there (the reference: padding_mode='circular' on its
        # nn.Conv2d's).  The convolution kernels only know zero padding: the image is extended by a wrapped halo of
        # _lib.TILE_HALO pixels (the network's receptive radius) and the centre is kept.  A sampling option: training is
        # unchanged.
        "tile": (False, False),
        # known-region conditioning (inpainting / outpainting): None or {s: (mask (H,W), x0 (3,H,W))}, fp32, on the sample's
        # device.  At a scale with an entry every reverse step overwrites the pixels whose mask is 1 with the
        # forward-diffused known image `x0` of the step's noise level, inside the step kernel (sinddm_sample_chain_keep);
        # values between 0 and 1 blend.  A sampling option, like `tile`; not available with CLIP guidance.
        "keep_maps": None,
        # per-pixel edit strength: False, or True -- the mask of every `keep_maps` entry is then a HOLD LEVEL h in [0, 1]
        # (1 - strength; functions.hold_pyramid) and a reverse step that lands on level u of a run whose top level is t_top
        # keeps the pixels with  h >= 1 - (u + 1) / (t_top + 1)  (functions.gate_thresholds; sinddm_sample_chain_gate): a
        # pixel is pinned to the forward-diffused known image down to its own level and left to the model from there --
        # SDEdit per pixel.  No soft blend; {0, 1} maps give the ungated run bit for bit.  Needs the scale's `keep_maps`
        # entry; a sampling option like `keep_maps`, not stored in checkpoints; not available with CLIP guidance.
        "keep_gated": False,
        # windowed known-region sampling: None, or a margin in pixels (an int >= 0).  A scale with a `keep_maps` entry is then
        # run on one window per sample -- the bounding box of its free pixels (mask / hold level < 1) grown by the margin,
        # functions.keep_windows -- and every draw is the full run's at the element's absolute position
        # (sinddm_normal_fill_window), so with a margin >= _lib.TILE_HALO, the receptive radius, the image of a seed is the
        # full run's image; everything outside the windows is the kept value, in closed form.  A run costs
        # what its hole costs.  A scale whose window spans it runs as ever.  Needs the scale's `keep_maps` entry; not with
        # `tile`, `layout_maps`, CLIP guidance or `noise_fn` (NOT_BUILT).  Not stored in checkpoints.
        "keep_window": None,
        # per-sample noise seeds: None (the draws come from torch's generators, as ever), a sequence of B ints in [0, 2^63)
        # (one seed per sample, used at every scale) or a [n_scales][B] nested sequence (row s at scale s; `vary_seeds`).
        # With seeds every N(0,1) draw of sample b -- initial, re-noise, every reverse step -- is a function of
        # (seed of b, noise_stream_id, element index inside the sample) alone: the sample does not depend on its batch, its
        # position in it, the two-stream split or the rank that runs it.  Not together with `noise_fn`.
        "sample_seeds": None,
        # seed blending: None, or (keys, weights) -- two [B][K] nested sequences, or [n_scales][B][K] like `sample_seeds`
        # (`mix_from_scale`) -- K <= 4 seeds in [0, 2^63) and K finite weights per sample whose squares add up to 1.  Every
        # N(0,1) draw of sample b is then  sum_k weights[b][k] * (the draw sample_seeds = keys[b][k] would give):  N(0,1)
        # again, and a function of the row alone, like a seeded sample.  Rows on an arc interpolate between two samples
        # (`interp_seeds`), rows on a circle make a closed loop (`loop_seeds`).  Not together with `sample_seeds` or
        # `noise_fn`; not with CLIP guidance.
        "seed_mix": None,
        # RePaint's resampling for known-region sampling: None or (R, J), both >= 1.  At anchor levels (multiples of J) the run
        # jumps back up by J levels and comes down again, until the stretch has been walked R times (the schedule:
        # functions.resample_schedule; the upward move: sinddm_sample_chain_resample).  R = 1 is None.  A sampling option,
        # like `keep_maps` (which it is meant for, and does not require); not available with CLIP guidance.
        "resample": None,
        # layout conditioning (paint-to-image): None or {s: (3, H_s, W_s) fp32 tensor on the sample's device}.  At a scale with
        # an entry, every reverse step with t >= layout_t_min pulls the low spatial frequencies of the predicted clean image
        # towards the layout's, with strength layout_strength in [0, 1]; "low" is the band below the block size
        # layout_down[s] (1 ... 64; functions.layout_blocks gives one physical band for all scales).  Strength and t_min are
        # one number or a dict per scale.  The contract: include/sinddm_hip.h (sinddm_layout_opts).  A sampling option like
        # `keep_maps`; not available with CLIP guidance or together with `resample`.
        "layout_maps": None,
        "layout_down": {},
        "layout_strength": 1.0,
        "layout_t_min": 0,
        # per-sample conditioning: a batch of B independent edit jobs per run.  Every map above may carry a leading batch
        # dimension -- keep_maps[s] = (mask (H,W) or (B,H,W), x0 (3,H,W) or (B,3,H,W)), the two independent of each other;
        # layout_maps[s] (3,H,W) or (B,3,H,W) -- and sample b is then conditioned on row b alone, whatever its position in
        # the batch, the two-stream split or the rank that runs it (sinddm_sample_chain_batch).  `layout_gain`: None or B
        # floats in [0, 1], sample b's factor on the layout strength.  `roi_bbs_batch` / `roi_target_patch_batch`: None or
        # B box lists / B patch lists (each what `roi_bbs` / `roi_target_patch` is for the whole batch; without the
        # second, every sample takes `roi_target_patch`).  The t schedule, `resample`, `tile`, `layout_down` and
        # `layout_t_min` stay one per run.
        "layout_gain": None,
        "roi_bbs_batch": None,
        "roi_target_patch_batch": None,
        # few-step sampling.  `sample_steps`: None (the network is evaluated at every level of every scale, as in the
        # reference), an int (at most that many evaluations per scale) or one value per scale (None: every level).
        # `sample_spacing`: which levels are kept -- 't' equally spaced in t, 'logsnr' equally spaced in log kappa
        # (functions.stride_schedule).  `solver_order`: 1 the step as it is (at a scale > 0 the DDIM form with SinDDM's
        # re-blur mix, at scale 0 the DDIM form with `eta`), 2 the second-order multistep step on top of it
        # (sinddm_sample_chain_solver).  `eta`: the noise of a scale-0 step as a share of the posterior's, 1.0 the
        # reference's DDPM step, 0 deterministic; `omega` stays the knob of the finer scales.  Sampling options like `tile`;
        # not stored in checkpoints; not with CLIP guidance or `resample`; order 2 not with `layout_maps`.
        "sample_steps": None,
        "sample_spacing": 't',
        "solver_order": 1,
        "eta": 1.0,
        # optional noise hook for parity tests: fn(kind, shape, s, t, device) -> tensor
        "noise_fn": None,
        # replay aid: when set to a list, every host-side draw ('init' / 'renoise', the tensor itself) and every fused
        # run of reverse steps (('chain', s, seed, [t...]): the in-kernel draws are sinddm_normal_fill(seed, i)) is logged
        "draw_log": None,
        "two_streams": True,       # coarse scales as two half-batches on two streams (sinddm_sample_chain2)
        "chain_noise": False,      # True: runs with a `noise_fn` take the chain call too (draws handed over as buffers)
        "chain_guided": True,      # False: ROI-guided runs take the step-by-step route (A/B measurements, bisecting)
        # ROI guidance (reference models.py:430-431): True -- at every scale but the finest the predicted clean image is pulled
        # towards `roi_target_patch` inside the boxes `roi_bbs` (or sample b's `roi_bbs_batch[b]`), which stay plain state.
        "roi_guided_sampling": False,
        # CLIP guidance (reference models.py:367-431): True -- the guidance branch of p_mean_variance runs, in eager torch
        # ops, against `clip_model` and the rest of the reference's CLIP state, which stays plain state.
        "clip_guided_sampling": False,
    }


SAMPLING_OPTIONS = frozenset(sampling_defaults())


def refuse(d, opt: str, other: str, on: Optional[bool] = None):
    """Raises NotImplementedError for the pair (opt, other) of NOT_BUILT when `other` is on (`on`; None: as `d` has it).  The
    readers of the options (`_keep_entry`, `_layout_entry`, `_resample_cfg`, `_few_step_cfg`, `_mix_for`) call it where they
    have always raised, `RunPlan` for what only a whole run or a single step shows."""
    if _ON[other](d) if on is None else on:
        raise NotImplementedError(NOT_BUILT[opt, other])


@dataclass
class Step:
    """One reverse step of a run."""
    pos: int                                   # position in the (expanded) run: the stream id of its draws
    t: int                                     # the level the network is evaluated at
    land: int                                  # the level the step lands on (-1: the clean image)
    k: _lib.StepCoefs
    ab: Tuple[float, float]                    # forward scalars of the known image at `land` ((1, 0) without keep maps)
    jump_to: Optional[int]                     # the level a resampling jump takes the step's output back up to, or None
    jump: Optional[_lib.JumpCoefs]
    g: float                                   # strength of the layout pull (0: the step is not conditioned)
    q: Optional[float]                         # multistep factor (None: a first-order run)
    thr: Optional[float] = None                # gate threshold in (0, 1], an fp32 value (None: the run is not gated)


class RunPlan:
    """The reverse steps `t_seq` of scale s on `img` with the options `d` carries; `at` = (step_pos, jump_to, land, q[, t_top])
    makes it the plan of the ONE step `t_seq = [t]` as `_p_sample_host_t` is handed it (`t_top`: the highest level of the run the
    step belongs to, which a gated step needs), else the schedule is resolved from `d`.
    Attributes: `steps` (the records), `t_seq` / `jump_to` (the expanded walk; `jump_to` None without resampling), `halo`,
    `roi` (ew, ec) / `keep` (mask, x0) / `lay` (layout, N, strength, t_min) or None each, `per` (which of edit, keep mask, keep x0,
    layout hold a slice per sample), `gain` (fp32 numpy or None), `xt` (x-tilde or None), `order2`, `gated` (`keep_gated`: every
    record carries `thr`, functions.gate_thresholds of its `land` and the run's top level before any resampling expansion),
    `noise` (kind, payload) with kind 'recorded' / 'seeds' / 'mix' / 'torch' / 'window' (None for a single step: its caller
    draws), `window` (functions.keep_windows of the run's free pixels under `keep_window`: (h, w, origins), or None -- not
    asked for, no free pixel, a window that spans the scale, a single step -- which is today's run field by field), `win`
    (None; on the cropped copy of the plan that `_run_steps` runs, the models._KeepWindow that makes its draws) and `full_hw`,
    the sample's own (H, W).

    The windowed run (`window` set): `_run_steps` gathers every input through the per-sample windows, runs the same steps on
    the (B, 3, h, w) tensors and scatters the result into the value the full run leaves outside them.  Its noise kind is
    'window': every draw is sinddm_normal_fill_window at the step's stream id, i.e. the draw the full run of `sample_seeds`
    or `seed_mix` makes at the element's ABSOLUTE position; the payload is (keys [B][K], weights [B][K] or None for plain
    seeds).  An UNSEEDED windowed run has payload None here: `_run_steps` draws B fresh 62-bit per-sample seeds from torch's
    CPU generator and keys every sample on its own -- it is therefore unrelated to the unseeded full run of the same
    torch.manual_seed (which keys the whole batch on one seed and the batch-flat index), but windowed runs of one
    torch.manual_seed agree with each other.

    Everything is validated here, in this order; each reader raises ValueError for a malformed option, SinddmError for a map
    that does not match `img`, and NotImplementedError (NOT_BUILT) where noted:
      1. a single step (`at`): strided or multistep (with CLIP, a jump), a jump (with CLIP)
      2. `_few_step_cfg` (with CLIP, resample), then functions.stride_schedule and `_solver_q`
      3. `_layout_entry` (with CLIP, resample); the entry is dropped when no step of the run pulls; then with order 2 / a jump
      4. `_resample_cfg` (with CLIP), then functions.resample_schedule
      5. `_seeds_for`, `_mix_for` (with CLIP): the noise source
      6. `keep_gated` (with CLIP), `_keep_entry` (with CLIP); `keep_gated` without keep maps for the scale, or on a single
         step without `t_top`: ValueError
      7. `roi_edit_maps` and its batch, `_layout_gain_for`
      8. the per-step scalars; x-tilde must be set when a step reads it"""

    def __init__(self, d, img, s: int, t_seq, *, at=None, clip_denoised: bool = True):
        s, t_seq = int(s), [int(t) for t in t_seq]
        B, clip = int(img.shape[0]), bool(d.clip_guided_sampling)
        pos0, j, land, q1, t_top = (tuple(at) + (None,))[:5] if at is not None else (0, None, None, None, None)
        if at is None and t_seq:
            t_top = max(t_seq)                                 # (of the run as handed over: before striding and resampling)
        if land is not None or q1 is not None:
            refuse(d, "strided_step", "clip_or_jump", clip or j is not None)
        if j is not None:
            refuse(d, "resample", "clip")
        lands, q, jump_to = ([f(v)] if v is not None else None for f, v in ((int, land), (float, q1), (int, j)))
        few = d._few_step_cfg(s) if at is None else None
        if few is not None and t_seq:
            t_seq, lands = stride_schedule(t_seq, few[0] if few[0] is not None else len(t_seq), few[1],
                                           d._kappa(s) if few[1] == 'logsnr' else None)
            q = d._solver_q(s, t_seq, lands) if few[2] == 2 else None
        lay = d._layout_entry(s, img)
        g = layout_strengths(t_seq, lay[2], lay[3]) if lay is not None else None
        if lay is not None and any(v > 0.0 for v in g):
            refuse(d, "layout_maps", "solver_order", q is not None)
            refuse(d, "layout_maps", "resample", jump_to is not None)
        else:
            lay = None
        rs = d._resample_cfg() if at is None else None
        if rs is not None:
            t_seq, jump_to = resample_schedule(t_seq, *rs)
        self.noise = None
        if at is None:
            seeds, mix = d._seeds_for(s, B), d._mix_for(s, B)
            self.noise = (("recorded", None) if d.noise_fn is not None else ("seeds", seeds) if seeds is not None
                          else ("mix", mix) if mix is not None else ("torch", None))
        windowed = at is None and d.keep_window is not None
        if windowed:
            refuse(d, "keep_window", "clip")
        gated = bool(d.keep_gated)
        if gated:
            refuse(d, "keep_gated", "clip")
        keep = d._keep_entry(s, img)
        if gated and keep is None:
            raise ValueError(f"keep_gated without keep_maps for scale {s}: there is no known region to gate")
        if gated and t_seq and t_top is None:
            raise ValueError("keep_gated: a single step needs t_top, the highest level of its run")
        self.window, self.win, self.full_hw = None, None, (int(img.shape[-2]), int(img.shape[-1]))
        if windowed:
            self.window = self._window_for(d, s, keep, lay, B)
            if self.window is not None:
                src = self.noise[1]
                self.noise = ("window", None if src is None else ([[int(v)] for v in src], None) if self.noise[0] == "seeds"
                              else (src[0], src[1]))
        roi = None
        if d.roi_guided_sampling and s < d.n_scales - 1 and not clip:       # models.py:430-431 (the CLIP step edits on its own)
            roi = d.roi_edit_maps(s, int(img.shape[-2]), int(img.shape[-1]), img.device)
            if roi[0].dim() == 3 and roi[0].shape[0] != B:                 # (raw pointers: B slices are read)
                raise ValueError(f"roi_bbs_batch has {roi[0].shape[0]} box lists, the batch {B} samples")
        gain = d._layout_gain_for(B, "cpu") if lay is not None else None
        self.s, self.t_seq, self.jump_to, self.halo, self.order2 = s, t_seq, jump_to, d._tile_halo(), q is not None
        self.roi, self.keep, self.lay, self.gain = roi, keep, lay, gain.numpy() if gain is not None else None
        self.per = (int(roi is not None and roi[0].dim() == 3), int(keep is not None and keep[0].dim() == 3),
                    int(keep is not None and keep[1].dim() == 4), int(lay is not None and lay[0].dim() == 4))
        tab, jt = d._coef_table(s, clip_denoised), d._jump_table(s) if jump_to is not None else None
        ab_tab = d._keep_ab_table() if keep is not None else None
        self.gated = gated
        lands_all = [t - 1 for t in t_seq] if lands is None else list(lands)
        thr = gate_thresholds(lands_all, t_top) if gated and t_seq else None
        self.steps = []
        for i, t in enumerate(t_seq):
            u = lands_all[i]
            l2 = jump_to[i] if jump_to is not None else None
            self.steps.append(Step(
                pos=pos0 + i, t=t, land=u,
                k=tab[t] if lands is None else d.step_coefs_to(t, u, s, clip_denoised, d.eta),
                # (row l + 1 holds the forward scalars of level l, row 0 those of the clean image)
                ab=tuple(float(v) for v in ab_tab[u + 1]) if keep is not None else (1.0, 0.0),
                jump_to=l2, jump=_lib.JumpCoefs(1, *jt(t - 1, l2)) if l2 is not None else None,
                g=g[i] if lay is not None else 0.0, q=q[i] if q is not None else None,
                thr=float(thr[i]) if thr is not None else None))
        self.xt = None
        if not clip and any(st.k.mode != 0 for st in self.steps):
            if d.img_prev_upsample is None:
                raise _lib.SinddmError("img_prev_upsample is not set (call sample_via_scale / p_sample_via_scale_loop)")
            self.xt = d.img_prev_upsample.contiguous()

    @staticmethod
    def _window_for(d, s: int, keep, lay, B: int):
        """functions.keep_windows of the run under `keep_window`, after its refusals."""
        margin = d.keep_window
        if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0:
            raise _lib.SinddmError(f"keep_window = {margin!r}: None or a margin, an integer >= 0")
        if keep is None:
            raise _lib.SinddmError(f"keep_window without keep_maps for scale {s}: there is no known region to window around")
        refuse(d, "keep_window", "tile", any(d.tile))
        refuse(d, "keep_window", "layout_maps", lay is not None)
        refuse(d, "keep_window", "noise_fn", d.noise_fn is not None)
        return keep_windows(keep[0] < 1, margin, batch=B)

    def log_entry(self, seed: int):
        """The `draw_log` entry of the run on the chain route with in-kernel draws (`seed`: the torch-seeded run's): draw i is
        sinddm_normal_fill over the sample (the EXTENDED one when tiled) at stream i, a jump's second draw 2^31 above it.  A
        windowed run: ("chain_window", s, seeds or (keys, weights), t list, jump targets or None, (h, w), origins) -- the draws
        of the seeded run's entry, of which the window is taken."""
        kind, src = self.noise
        t, jumps = list(self.t_seq), list(self.jump_to) if self.jump_to is not None else None
        if kind == "window":                                   # (`seed` unused: the payload holds the keys, drawn or given)
            key = [k[0] for k in src[0]] if src[1] is None else (src[0], src[1])
            return ("chain_window", self.s, key, t, jumps, tuple(self.window[:2]), self.window[2])
        if kind == "mix":
            return ("chain_mix", self.s, (src[0], src[1]), t, jumps)
        key = list(src) if kind == "seeds" else seed
        if jumps is not None:
            return ("chain_resample", self.s, key, t, jumps)
        if kind == "seeds":
            return ("chain_seeds", self.s, key, t)
        return ("chain_tile", self.s, key, t, self.halo) if any(self.halo) else ("chain", self.s, key, t)


def pack_steps(plan: RunPlan, i0: int, k: int):
    """The host arrays of the steps [i0, i0 + k) of `plan` as a chain call takes them: `coefs`, `tl`, and `ab` (2 per step), `jumps`,
    `g`, `q`, `thr` -- None each when the run does not have the option."""
    st = plan.steps[i0:i0 + k]
    arr = lambda ctype, vals: (ctype * len(vals))(*vals)
    return SimpleNamespace(
        coefs=arr(_lib.StepCoefs, [r.k for r in st]), tl=arr(C.c_int, [r.t for r in st]),
        ab=arr(C.c_float, [v for r in st for v in r.ab]) if plan.keep is not None else None,
        jumps=arr(_lib.JumpCoefs, [_lib.JumpCoefs(0, 0.0, 0.0, 0.0) if r.jump is None else r.jump for r in st])
        if plan.jump_to is not None else None,
        g=arr(C.c_float, [r.g for r in st]) if plan.lay is not None else None,
        q=arr(C.c_float, [r.q for r in st]) if plan.order2 else None,
        thr=arr(C.c_float, [r.thr for r in st]) if plan.gated else None)
