#!/usr/bin/env python3
"""Command line of the MI355X SinDDM hot-path build: same flags as the reference's main.py
(reference main.py:13-58) for the modes that run on the hot path: `train`, `sample`, `style_transfer`,
`harmonization` and `roi`, plus the modes the reference does not have (below).

    python main.py --scope balloons --mode train  --dataset_folder ./datasets/balloons/ --image_name balloons.png
    python main.py --scope balloons --mode sample --dataset_folder ./datasets/balloons/ --image_name balloons.png \
                   --load_milestone 12 --sample_batch_size 16 [--scale_mul 2 4]

Multi-GPU sampling: launch one process per GPU with torchrun; the sample batch is sharded over the
ranks as independent chains and all-gathered (RCCL over xGMI):
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 main.py --mode sample ...

`style_transfer` / `harmonization` (reference main.py:296-322) drive `MultiscaleTrainer.image2image`; `roi`
(main.py:257-294) drives `roi_guided_sampling` -- the reference picks the boxes with a cv2 GUI, here they come from
`--roi_target y x h w` and `--roi_bbs y x h w [y x h w ...]` (finest-scale pixel coordinates).
`--tile {none,x,y,xy}` (no reference flag) samples with borders that wrap around on the named axes: tileable textures,
cylindrical panoramas (`--tile x --scale_mul 1 4`).  All five modes honour it.
`--train_tile {none,x,y,xy}` (no reference flag) TRAINS with borders that wrap around on the named axes, so the weights have seen
the seam `--tile` later asks them for; the intended pairing is `--mode train --tile xy --train_tile xy`.  It changes the
training step only (`--tile` alone keeps sampling from zero-padding-trained weights), and is not stored in checkpoints.
`--train_mask FILE` (no reference flag) TRAINS on the white part of FILE only (white = train on, black = ignore: a scratch, a
watermark, an object to remove; the file is brought to the finest scale's size the way `--mask_path` is): the loss becomes the
weighted mean over the valid pixels of every scale, and with `--train_mask_fill mean` (the default; `image` leaves the picture
alone) the hole pixels of the training images are replaced by the mean of the valid ones.  `--train_mask_grow N [N ...]` (one
value, or one per scale; default 0) grows the hole by N pixels of each scale before the loss is switched off.  The network's
receptive field is a square of radius 16, so with N = 16 the weights provably never see the hole; coarse scales may not survive
that (a scale left without a valid pixel is an error), so give one value per scale, for example `0 0 4 8 16`.  The pyramid
files on disk stay as they are: their down-scaling smears hole content a few pixels outward, which is what N is for.  The
intended pairing is `--mode train --train_mask hole.png`, then `--mode inpaint --mask_path hole.png`.  Like `--train_tile`
the flags change the training step only (the other modes accept and ignore them) and are not stored in checkpoints.
`--train_crop H W` (no reference flag) TRAINS on random windows: at every scale larger than H x W each sample of a batch
sees its own window of at most H x W pixels, so a step costs what the window costs, not what the image costs.
`--train_crop_margin N` (default 0) switches the loss off within N pixels of every window side that is not an image border;
with N = 16, the network's receptive radius, a cropped step is provably a masked full-image step, and the window origins are
drawn so that border pixels are supervised as often as interior ones.  Used with `--mode train` only, not stored in
checkpoints, and not together with `--train_tile`.
`inpaint` and `outpaint` (no reference modes) keep some pixels exactly and generate the rest to fit, by replacing the
known region after every reverse step inside the step kernels: `--mode inpaint --mask_path FILE [--soft_mask]` fills the
black part of the mask (white = keep the training image's pixel; the file is brought to the finest scale's size);
`--mode outpaint --scale_mul h w [--anchor y x]` grows the canvas around the training image.  `--resample R --jump_length J`
(both modes; defaults 1 1 = no jumps) add RePaint's resampling: at every noise level that is a multiple of J the run jumps
back up by J levels and comes down again, R times in all, so that the generated region is shaped with the known one in view.
`--keep_window [N]` (`inpaint`, `outpaint`, `edit`; default N = 16) runs every scale on the window around the pixels that may
change -- their bounding box grown by N -- with the noise of the full run: with N >= 16, the network's receptive radius, the
picture of a seed is the one the full run draws, and the run costs what its hole costs.  Not with `--tile`.
`edit` (no reference mode) edits a picture with a strength per pixel: `--mode edit --edit_map FILE [FILE ...] [--edit_image FILE
[FILE ...]]`.  The map is a gray picture brought to the finest target size, read as value / 255: black = leave the pixel alone,
white = redraw it freely, gray = re-noise it to that share of every scale's levels and let the model take it from there (each
pixel its own SDEdit start level: "leave the sky, retouch the trees a little, redraw the foreground").  `--edit_image` is the
picture being edited (a path, or a name inside the dataset folder; default: the training image).  Inside the step kernels a
pixel stays pinned to the forward-diffused picture until the run is down to its level (`keep_gated`: still one library call per
scale); a black-and-white map is `inpaint` with the inverted mask, bit for bit.  `--tile`, `--seeds` and the blend flags,
`--resample` / `--jump_length`, `--sample_steps` / `--solver_order` and `--scale_mul` (with `--edit_image`) apply.  (The
reference's `--strength` is a CLIP flag: hence `--edit_map`.)
`--sample_steps N [N ...]` (no reference flag; one value, or one per scale) evaluates the network at no more than N levels per
scale instead of all of them, `--sample_spacing {t,logsnr}` chooses which, `--solver_order 2` takes the second-order multistep
step that makes few steps accurate, `--eta F` scales the noise of a scale-0 step (1 = the reference's, 0 = deterministic).  Every
sampling mode honours them, except together with `--resample` and, for `--solver_order 2`, `paint2image`.
`paint2image` (no reference mode) redraws a rough picture -- a scribble, a colour sketch, a blurred photo -- in the training
image's texture while its layout stays put: `--mode paint2image --input_image FILE [--layout_down N] [--layout_strength G]
[--layout_t_min T] [--layout_scales A B]` pulls the low spatial frequencies (the band below N pixels of the finest scale) of
every step's predicted clean image towards the picture's, with strength G in [0, 1], at the steps with t >= T of the scales
A ... B (default: all).  FILE (a path, or a name inside the dataset folder) is brought to the finest target size.
`--seeds S [S ...]` (one per sample of the batch) or `--seed_base N` (seeds N ... N + batch - 1) give every sample its own
noise seed (no reference flag: the reference never seeds its generator): the image of a seed is the same at any batch size,
position in the batch and number of GPUs.  `--vary_from_scale S` keeps the given seeds below scale S and derives fresh
ones per sample from S on: `--seeds 17 17 17 17 --vary_from_scale 3` makes four variations of one coarse layout.
`--interp_seeds A B` and `--loop_seeds BASE A B [--loop_radius R]` (no reference flags; in place of `--seeds`) blend seeds:
every noise draw of frame b is a fixed unit-norm combination of the draws of the named seeds, so the frames walk from sample A
to sample B, or around sample BASE on a closed circle of radius R (default 0.5).  `--frames N` is the batch size and frame b
is sample b; `--blend_from_scale S` lets the scales below S use each frame's first seed alone (a shared coarse layout with
detail that moves); `--gif MS` also writes the finest scale's frames as one animated GIF, MS milliseconds per frame, a loop
repeating for ever.  Every sampling mode honours them.
A batch of independent jobs: `--mask_path`, `--input_image`, `--edit_map`, `--edit_image` and `--layout_strength` take one or more
values and `--anchor` one or more pairs.  With N > 1 values the batch size must be a multiple of N and sample b gets value b % N (so `--seeds` sweeps
line up: `--sample_batch_size 8 --mask_path a.png b.png --seed_base 0` fills each hole four times); every sample is then
conditioned on its own maps inside the one chain call per scale.  One value is the command line as it was.
`evaluate` (no reference mode) measures what the samples copy: `--mode evaluate [--eval_patch {3,5,7}] [--eval_scale S]` draws a
batch the way `--mode sample` does (`--seeds`, `--tile`, `--scale_mul`, `--sample_steps` ... apply), computes the patch
nearest-neighbour field between the batch of scale S (default: the finest) and that scale's training image in both
directions, prints fidelity, coherence, coverage (and seam under `--tile`) and writes `patch_report.json` to the results folder.
`--patch_refine ITERS` (no reference flag; `--mode sample` and `--mode evaluate` only) acts on that report: after the chain of
every scale in `--patch_refine_scales A B` (default: all) the batch is snapped to that scale's training image by ITERS
patch-vote iterations -- every `--patch_refine_patch {3,5,7}` patch is replaced by its nearest training patch and every pixel
becomes the mean of the patches that cover it (the EM step of GPNN) -- before the next scale re-noises and redraws it.
`--patch_refine_alpha A` ranks with GPNN's completeness normalisation D / (A 3P^2 + min D) (coverage in place of plain
fidelity); `--patch_refine_blend B` in [0, 1] moves only the share B of the way.  Off by default.
`--patch_refine_radius R` (0 .. 16) searches exhaustively only at the first refined scale: every later search looks in a
window of R positions around the previous field, carried from iteration to iteration and from scale to scale.
`score` (no reference mode) asks the MODEL: `--mode score [--input_image FILE ...] [--score_levels N] [--score_draws R]
[--score_scales A B]` evaluates the training L1 loss |z - eps| per pixel with the trained weights, at N noise levels per scale
(default 10, spread over the levels the scale was trained on) and R noise draws per level (default 4; `--seeds` names them), on
the scales A ... B (default: all).  Without `--input_image` it scores the training pyramid: `score_report.json` is the
checkpoint's per-scale / per-level loss table.  With pictures (paths, or names inside the dataset folder, brought to the finest
size) each is scored side by side with the training image, `score_s{S}.png` shows the maps, and `score_edit_map.png` -- the
finest map normalised against the training image's own (median -> 0, maximum -> 1) -- is a gray strength map that
`--mode edit --edit_map score_edit_map.png` takes as it is: redraw what the model finds implausible, keep the rest.  `--tile`
is refused (the wrapped-halo score is not built); `--train_mask` keeps the hole out of the score.
The CLIP-guided modes (clip_content, clip_style_*, clip_roi; main.py:153-255) are not wired to the command line: CLIP
itself is outside this build.  Their drivers exist (`MultiscaleTrainer.clip_sampling` / `clip_roi_sampling`, the guidance
branch of `p_mean_variance`) and take any scorer with the reference's ClipExtractor interface.
"""
import argparse
import os

import torch

from sinddm_amd.functions import create_img_scales
from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
from sinddm_amd.trainer import MultiscaleTrainer


# (flag, default, type, nargs) -- names, defaults and types follow reference main.py:13-58 so existing
# command lines keep working; flags that only feed the un-built guided modes are accepted and ignored.
_FLAGS = [
    ("scope", "forest", str, None), ("mode", None, str, None),
    ("input_image", "seascape_composite_dragon.png", str, None), ("start_t_harm", 5, int, None),
    ("start_t_style", 15, int, None), ("harm_mask", "seascape_mask_dragon.png", str, None),
    ("clip_text", "Fire in the Forest", str, None), ("fill_factor", None, float, None),
    ("strength", None, float, None), ("roi_n_tar", 1, int, None),
    ("dataset_folder", "./datasets/forest/", str, None), ("image_name", "forest.jpeg", str, None),
    ("results_folder", "./results/", str, None),
    ("dim", 160, int, None), ("scale_factor", 1.411, float, None), ("timesteps", 100, int, None),
    ("train_batch_size", 32, int, None), ("grad_accumulate", 1, int, None), ("train_num_steps", 120001, int, None),
    ("save_and_sample_every", 10000, int, None), ("avg_window", 100, int, None), ("train_lr", 1e-3, float, None),
    ("sched_k_milestones", [20, 40, 70, 80, 90, 110], int, "+"), ("load_milestone", 0, int, None),
    ("sample_batch_size", 16, int, None), ("scale_mul", [1, 1], float, "+"), ("sample_t_list", None, int, "+"),
    ("device_num", 0, int, None), ("omega", 0, float, None), ("loss_factor", 1, float, None),
    # non-interactive stand-ins for the cv2.selectROI dialogs of the reference's `roi` mode
    ("roi_target", None, int, "+"), ("roi_bbs", None, int, "+"),
    # known-region sampling: the mask file of `inpaint`, the placement of the training image on the canvas of `outpaint`
    ("mask_path", None, str, None), ("anchor", [0.5, 0.5], float, 2),
    # per-pixel edit strength: the gray strength map of `edit` (white = redraw freely, black = keep) and the picture it edits
    ("edit_map", None, str, None), ("edit_image", None, str, None),
]


class Jobs(list):
    """Several values of a per-job flag, one job each (a single value stays the scalar it always was)."""


class _OneOrMore(argparse.Action):
    """nargs='+': one value is stored as itself, several as `Jobs`."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values[0] if len(values) == 1 else Jobs(values))
        setattr(namespace, self.dest + "_given", True)          # (the flag was on the command line: a default never passes here)


class _Pairs(argparse.Action):
    """--anchor y x [y x ...]: one pair is stored as the flat [y, x], several as `Jobs` of pairs."""

    def __call__(self, parser, namespace, values, option_string=None):
        if len(values) % 2:
            parser.error(f"{option_string}: y x pairs expected, got {len(values)} values")
        pairs = [list(values[i:i + 2]) for i in range(0, len(values), 2)]
        setattr(namespace, self.dest, pairs[0] if len(pairs) == 1 else Jobs(pairs))


_PER_JOB = ("mask_path", "input_image", "layout_strength", "anchor", "edit_map", "edit_image")   # the flags that take one value per job


def job_values(value, batch_size):
    """A per-job flag for a batch: `Jobs` of N values -> the list of `batch_size` values, sample b gets value b % N; one
    value is returned as it is."""
    if not isinstance(value, Jobs):
        return value
    return [value[b % len(value)] for b in range(int(batch_size))]


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, dflt, typ, nargs in _FLAGS:
        kw = dict(default=dflt, type=typ)
        if nargs:
            kw["nargs"] = nargs
        if name in _PER_JOB:
            kw.update(nargs="+", action=_Pairs if name == "anchor" else _OneOrMore)
        p.add_argument("--" + name, **kw)
    p.add_argument("--sample_limited_t", action="store_true")
    # no reference flag (there: padding_mode='circular' on the nn.Conv2d's): borders that wrap around on the x axis (360-degree
    # panoramas), the y axis or both (seamlessly tileable textures) -- MultiScaleGaussianDiffusion.tile
    p.add_argument("--soft_mask", action="store_true")    # inpaint: blend with the area-averaged mask at coarse scales
    p.add_argument("--tile", choices=("none", "x", "y", "xy"), default="none")
    # the training half of --tile (MultiScaleGaussianDiffusion.train_tile): p_losses wraps the named axes around
    p.add_argument("--train_tile", choices=("none", "x", "y", "xy"), default="none")
    # the training half of `inpaint` (MultiScaleGaussianDiffusion.train_weights): the loss ignores the black part of the mask
    # crop training (MultiScaleGaussianDiffusion.train_crop / train_crop_margin): random windows per sample
    p.add_argument("--train_crop", type=int, nargs=2, default=None, metavar=("H", "W"))
    p.add_argument("--train_crop_margin", type=int, default=0, metavar="N")
    p.add_argument("--train_mask", type=str, default=None, metavar="FILE")
    p.add_argument("--train_mask_grow", type=int, nargs="+", default=[0], metavar="N")
    p.add_argument("--train_mask_fill", choices=("mean", "image"), default="mean")
    # no reference flags: per-sample noise seeds (MultiScaleGaussianDiffusion.sample_seeds) of every sampling mode
    g = p.add_mutually_exclusive_group()
    g.add_argument("--seeds", type=int, nargs="+", default=None)
    g.add_argument("--seed_base", type=int, default=None)
    # no reference flags: seed blending (MultiScaleGaussianDiffusion.seed_mix) of every sampling mode.  --frames N is the batch
    # size: frame b is sample b, an interpolation from sample A to sample B or a closed loop around sample BASE.
    g.add_argument("--interp_seeds", type=int, nargs=2, default=None, metavar=("A", "B"))
    g.add_argument("--loop_seeds", type=int, nargs=3, default=None, metavar=("BASE", "A", "B"))
    p.add_argument("--loop_radius", type=float, default=0.5)
    p.add_argument("--frames", type=int, default=None)
    p.add_argument("--blend_from_scale", type=int, default=0)
    p.add_argument("--gif", type=int, default=None, metavar="MS")      # also write the frames as one animated GIF, MS per frame
    p.add_argument("--vary_from_scale", type=int, default=None)
    # no reference flags: RePaint's resampling jumps of `inpaint` / `outpaint` (MultiScaleGaussianDiffusion.resample)
    p.add_argument("--resample", type=int, default=1)
    p.add_argument("--jump_length", type=int, default=1)
    # no reference flag: windowed known-region sampling of `inpaint` / `outpaint` / `edit` (MultiScaleGaussianDiffusion.keep_window)
    p.add_argument("--keep_window", type=int, nargs="?", const=16, default=None, metavar="N")
    # no reference flags: few-step sampling (MultiScaleGaussianDiffusion.sample_steps / sample_spacing / solver_order / eta)
    p.add_argument("--sample_steps", type=int, nargs="+", default=None)
    p.add_argument("--sample_spacing", choices=("t", "logsnr"), default="t")
    p.add_argument("--solver_order", type=int, choices=(1, 2), default=1)
    p.add_argument("--eta", type=float, default=1.0)
    # no reference flags: layout conditioning of `paint2image` (MultiscaleTrainer.paint2image)
    p.add_argument("--layout_down", type=int, default=8)
    p.add_argument("--layout_strength", type=float, default=1.0, nargs="+", action=_OneOrMore)
    p.add_argument("--layout_t_min", type=int, default=0)
    p.add_argument("--layout_scales", type=int, nargs=2, default=None)
    # no reference flags: the patch nearest-neighbour report of `evaluate` (MultiscaleTrainer.evaluate)
    p.add_argument("--eval_patch", type=int, choices=(3, 5, 7), default=7)
    p.add_argument("--eval_scale", type=int, default=None, metavar="S")
    # no reference flags: patch-vote refinement between the scales (MultiscaleTrainer.sample_scales(patch_refine=...))
    p.add_argument("--patch_refine", type=int, default=None, metavar="ITERS")
    p.add_argument("--patch_refine_patch", type=int, choices=(3, 5, 7), default=7)
    p.add_argument("--patch_refine_alpha", type=float, default=None, metavar="A")
    p.add_argument("--patch_refine_blend", type=float, default=1.0, metavar="B")
    p.add_argument("--patch_refine_scales", type=int, nargs=2, default=None, metavar=("A", "B"))
    p.add_argument("--patch_refine_radius", type=int, default=None, metavar="R")
    # no reference flags: the denoising-score maps of `score` (MultiscaleTrainer.score)
    p.add_argument("--score_levels", type=int, default=10, metavar="N")
    p.add_argument("--score_draws", type=int, default=4, metavar="R")
    p.add_argument("--score_scales", type=int, nargs=2, default=None, metavar=("A", "B"))
    return p


def parse_args(argv=None):
    """Parse the command line and resolve the seed flags: `args.seeds` becomes the list of `sample_batch_size` seeds (or
    stays None), `args.seed_mix` the [frames][K] blend tables of --interp_seeds / --loop_seeds (or None)."""
    p = build_parser()
    args = p.parse_args(argv)
    args.seed_mix = None
    if args.interp_seeds is not None or args.loop_seeds is not None:
        from sinddm_amd.models import interp_seeds, loop_seeds
        if args.frames is not None:
            args.sample_batch_size = args.frames
        try:
            if args.interp_seeds is not None:
                args.seed_mix = interp_seeds(*args.interp_seeds, args.sample_batch_size)
            else:
                args.seed_mix = loop_seeds(*args.loop_seeds, args.sample_batch_size, args.loop_radius)
        except ValueError as e:
            p.error(str(e))
        if args.blend_from_scale < 0:
            p.error("--blend_from_scale must be >= 0")
        if args.gif is not None and args.gif < 1:
            p.error("--gif MS must be >= 1")
    elif args.frames is not None or args.gif is not None or args.blend_from_scale != 0:
        p.error("--frames / --gif / --blend_from_scale need --interp_seeds or --loop_seeds")
    if args.seed_base is not None:
        args.seeds = [args.seed_base + b for b in range(args.sample_batch_size)]
    if args.seeds is not None:
        if len(args.seeds) != args.sample_batch_size:
            p.error(f"--seeds: {len(args.seeds)} seeds for --sample_batch_size {args.sample_batch_size}")
        if min(args.seeds) < 0 or max(args.seeds) >= 2 ** 63:
            p.error("--seeds / --seed_base: a seed must be in [0, 2^63)")
    elif args.vary_from_scale is not None:
        p.error("--vary_from_scale needs --seeds or --seed_base")
    if args.vary_from_scale is not None and args.vary_from_scale < 0:
        p.error("--vary_from_scale must be >= 0")
    if args.resample < 1 or args.jump_length < 1:
        p.error("--resample and --jump_length must be >= 1")
    if args.keep_window is not None:
        if args.mode not in ("inpaint", "outpaint", "edit"):
            p.error("--keep_window applies to --mode inpaint, outpaint and edit")
        if args.keep_window < 0:
            p.error("--keep_window N must be >= 0")
    if args.sample_steps is not None and min(args.sample_steps) < 1:
        p.error("--sample_steps must be >= 1")
    if min(args.train_mask_grow) < 0:
        p.error("--train_mask_grow must be >= 0")
    if args.train_crop is not None and min(args.train_crop) < 1:
        p.error("--train_crop H W must be >= 1")
    if args.train_crop_margin < 0:
        p.error("--train_crop_margin must be >= 0")
    if args.train_crop is not None and args.train_tile != "none":
        p.error("--train_crop does not go together with --train_tile: windows that wrap around the border are not built")
    if args.eta < 0.0:
        p.error("--eta must be >= 0")
    if not 1 <= args.layout_down <= 64:
        p.error("--layout_down must be in 1 ... 64")
    for g in (args.layout_strength if isinstance(args.layout_strength, Jobs) else [args.layout_strength]):
        if not 0.0 <= g <= 1.0:
            p.error("--layout_strength must be in [0, 1]")
    for name in _PER_JOB:
        v = getattr(args, name)
        if args.mode == "score" and name == "input_image":           # (the pictures `score` scores are not a sample batch)
            continue
        if isinstance(v, Jobs) and args.sample_batch_size % len(v):
            p.error(f"--{name}: {len(v)} values need --sample_batch_size to be a multiple of {len(v)}, got "
                    f"{args.sample_batch_size}")
    if args.layout_t_min < 0:
        p.error("--layout_t_min must be >= 0")
    if args.layout_scales is not None and not 0 <= args.layout_scales[0] <= args.layout_scales[1]:
        p.error("--layout_scales A B needs 0 <= A <= B")
    if args.eval_scale is not None and args.eval_scale < 0:
        p.error("--eval_scale must be >= 0")
    args.patch_refine_opt = None
    if args.patch_refine is None:
        if (args.patch_refine_patch != 7 or args.patch_refine_alpha is not None or args.patch_refine_blend != 1.0
                or args.patch_refine_scales is not None or args.patch_refine_radius is not None):
            p.error("--patch_refine_patch / _alpha / _blend / _scales / _radius need --patch_refine ITERS")
    else:
        if args.mode not in ("sample", "evaluate"):
            p.error(f"--patch_refine goes with --mode sample and --mode evaluate, not with --mode {args.mode}")
        if args.patch_refine < 1:
            p.error("--patch_refine ITERS must be >= 1")
        a, b = args.patch_refine_alpha, args.patch_refine_blend
        if a is not None and not (a > 0.0 and a != float("inf")):
            p.error("--patch_refine_alpha must be finite and > 0")
        if not 0.0 <= b <= 1.0:
            p.error("--patch_refine_blend must be in [0, 1]")
        sc = args.patch_refine_scales
        if sc is not None and not 0 <= sc[0] <= sc[1]:
            p.error("--patch_refine_scales A B needs 0 <= A <= B")
        args.patch_refine_opt = dict(iters=args.patch_refine, patch=args.patch_refine_patch, alpha=a, blend=b,
                                     scales=None if sc is None else (sc[0], sc[1]))
        if args.patch_refine_radius is not None:               # (absent: the option dict every earlier command line made)
            if not 0 <= args.patch_refine_radius <= 16:
                p.error("--patch_refine_radius R must be in 0 .. 16")
            args.patch_refine_opt["radius"] = args.patch_refine_radius
    args.score_images = None
    if args.mode == "score":
        if args.score_levels < 1 or args.score_draws < 1:
            p.error("--score_levels and --score_draws must be >= 1")
        if args.score_scales is not None and not 0 <= args.score_scales[0] <= args.score_scales[1]:
            p.error("--score_scales A B needs 0 <= A <= B")
        # (`score` scores the training pyramid alone unless --input_image is GIVEN: the flag's default is the reference's file
        # name of the i2i modes; _OneOrMore marks a flag that was on the command line)
        if getattr(args, "input_image_given", False):
            args.score_images = args.input_image
    if args.mode == "edit" and not args.edit_map:
        p.error("--mode edit needs --edit_map FILE (a gray picture: white = redraw freely, black = keep the pixel)")
    return args


def main():
    args = parse_args()
    seed_kw = dict(seeds=args.seeds, vary_from_scale=args.vary_from_scale)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    td = None
    if world > 1:
        import torch.distributed as td
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        td.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        args.device_num = local_rank
        torch.manual_seed(1234 + td.get_rank())      # every rank draws its own chains
    print('num devices: ' + str(torch.cuda.device_count()))
    device = f"cuda:{args.device_num}"
    if world == 1 and torch.cuda.is_available():
        torch.cuda.set_device(args.device_num)      # the HIP library launches on the CURRENT device's stream
    scale_mul = (args.scale_mul[0], args.scale_mul[1])
    sched_milestones = [val * 1000 for val in args.sched_k_milestones]
    results_folder = args.results_folder + '/' + args.scope

    # reference main.py:71-75.  Under torch.distributed only rank 0 writes the scale_i/ PNG pyramid; the others wait
    # and then only derive the sizes / losses from the files rank 0 wrote (create=False), so no rank ever opens a
    # half-written PNG.
    rank = 0
    if world > 1:
        rank = td.get_rank()
    if rank == 0:
        sizes, rescale_losses, scale_factor, n_scales = create_img_scales(
            args.dataset_folder, args.image_name, scale_factor=args.scale_factor, create=True, auto_scale=50000)
    if world > 1:
        td.barrier()
        if rank != 0:
            sizes, rescale_losses, scale_factor, n_scales = create_img_scales(
                args.dataset_folder, args.image_name, scale_factor=args.scale_factor, create=False, auto_scale=50000)
        td.barrier()

    model = SinDDMNet(dim=args.dim, multiscale=True, device=device)
    model.to(device)
    ms_diffusion = MultiScaleGaussianDiffusion(
        denoise_fn=model, save_interm=False, results_folder=results_folder, n_scales=n_scales,
        scale_factor=scale_factor, image_sizes=sizes, scale_mul=scale_mul, channels=3, timesteps=args.timesteps,
        train_full_t=True, scale_losses=rescale_losses, loss_factor=args.loss_factor, loss_type='l1', betas=None,
        device=device, reblurring=True, sample_limited_t=args.sample_limited_t, omega=args.omega).to(device)

    sample_t_list = ms_diffusion.num_timesteps_ideal[1:] if args.sample_t_list is None else args.sample_t_list

    mask_kw = {}
    if args.train_mask and args.mode in ('train', 'score'):                # (`score` keeps the hole out of its maps; the other modes never train: nothing to mask)
        import numpy as np
        from PIL import Image
        if len(args.train_mask_grow) not in (1, n_scales):
            raise SystemExit(f"--train_mask_grow: {len(args.train_mask_grow)} values for {n_scales} scales (give one, or one per "
                             "scale)")
        h, w = ms_diffusion.image_sizes[n_scales - 1]
        valid = torch.from_numpy((np.asarray(Image.open(args.train_mask).convert("L").resize((w, h), Image.NEAREST)) > 127)
                                 .astype(np.float32))
        mask_kw = dict(train_mask=valid, train_mask_fill=args.train_mask_fill,
                       train_mask_grow=args.train_mask_grow[0] if len(args.train_mask_grow) == 1 else list(args.train_mask_grow))

    if args.train_crop is not None and args.mode == 'train':               # (likewise: only training crops)
        mask_kw.update(train_crop=tuple(args.train_crop), train_crop_margin=args.train_crop_margin)

    trainer = MultiscaleTrainer(
        ms_diffusion, folder=args.dataset_folder, n_scales=n_scales, scale_factor=scale_factor, image_sizes=sizes,
        train_batch_size=args.train_batch_size, train_lr=args.train_lr, train_num_steps=args.train_num_steps,
        gradient_accumulate_every=args.grad_accumulate, ema_decay=0.995, fp16=False,
        save_and_sample_every=args.save_and_sample_every, avg_window=args.avg_window,
        sched_milestones=sched_milestones, results_folder=results_folder, device=device,
        train_tile=("y" in args.train_tile, "x" in args.train_tile), **mask_kw)

    # a sampling option (training is governed by --train_tile): every mode below samples with the EMA model
    trainer.ema_model.tile = ("y" in args.tile, "x" in args.tile)
    if args.sample_steps is not None:
        if len(args.sample_steps) not in (1, n_scales):
            raise SystemExit(f"--sample_steps: {len(args.sample_steps)} values for {n_scales} scales (give one, or one per scale)")
        trainer.ema_model.sample_steps = args.sample_steps[0] if len(args.sample_steps) == 1 else list(args.sample_steps)
    trainer.ema_model.sample_spacing, trainer.ema_model.solver_order, trainer.ema_model.eta = (
        args.sample_spacing, args.solver_order, args.eta)
    if args.load_milestone > 0:
        trainer.load(milestone=args.load_milestone)
    if args.seed_mix is not None:                                          # (a blend in place of seeds; the old command lines: untouched)
        from sinddm_amd.models import mix_from_scale
        if args.blend_from_scale > n_scales:
            raise SystemExit(f"--blend_from_scale {args.blend_from_scale} is past the {n_scales} scales")
        seed_kw = dict(seed_mix=mix_from_scale(args.seed_mix, args.blend_from_scale, n_scales) if args.blend_from_scale > 0
                       else args.seed_mix)
    # (without --patch_refine the argument is not passed at all: the old command lines run the old call)
    refine_kw = {} if args.patch_refine_opt is None else dict(patch_refine=args.patch_refine_opt)
    frames = None                                                          # the per-scale batches of the sampling modes
    if args.mode == 'train':
        trainer.train()
        trainer.sample_scales(scale_mul=(1, 1), custom_sample=True, image_name=args.image_name,
                              batch_size=args.sample_batch_size, custom_t_list=sample_t_list, **seed_kw)
    elif args.mode == 'sample':
        frames = trainer.sample_scales(scale_mul=scale_mul, custom_sample=True, image_name=args.image_name,
                              batch_size=args.sample_batch_size, custom_t_list=sample_t_list, save_unbatched=True,
                              **refine_kw, **seed_kw)
    elif args.mode in ('style_transfer', 'harmonization'):                 # reference main.py:296-322
        i2i_folder = os.path.join(args.dataset_folder, 'i2i')
        start_s = n_scales - 1                                             # start the diffusion at the last scale
        start_t = args.start_t_style if args.mode == 'style_transfer' else args.start_t_harm
        use_hist = args.mode == 'style_transfer'
        custom_t = [0] * (n_scales - 1) + [start_t]
        trainer.ema_model.reblurring = True
        frames = trainer.image2image(input_folder=i2i_folder, input_file=args.input_image, mask=args.harm_mask,
                            hist_ref_path=f'{args.dataset_folder}scale_{start_s}/', batch_size=args.sample_batch_size,
                            image_name=args.image_name, start_s=start_s, custom_t=custom_t, scale_mul=(1, 1),
                            device=device, use_hist=use_hist, save_unbatched=True, auto_scale=50000, mode=args.mode,
                            **seed_kw)
    elif args.mode == 'roi':                                               # reference main.py:257-294
        if not args.roi_target or len(args.roi_target) != 4 or not args.roi_bbs or len(args.roi_bbs) % 4:
            raise SystemExit("--mode roi needs --roi_target y x h w and --roi_bbs y x h w [y x h w ...]")
        bbs = [list(args.roi_bbs[i:i + 4]) for i in range(0, len(args.roi_bbs), 4)]
        frames = trainer.roi_guided_sampling(custom_t_list=sample_t_list, target_roi=list(args.roi_target), roi_bb_list=bbs,
                                    save_unbatched=True, batch_size=args.sample_batch_size, scale_mul=scale_mul, **seed_kw)
    elif args.mode == 'inpaint':
        if not args.mask_path:
            raise SystemExit("--mode inpaint needs --mask_path FILE (white = keep the training image's pixel, black = fill)")
        import numpy as np
        from PIL import Image
        h, w = ms_diffusion.image_sizes[n_scales - 1]
        load = lambda f: torch.from_numpy((np.asarray(Image.open(f).convert("L").resize((w, h), Image.NEAREST)) > 127)
                                          .astype(np.float32))
        paths = job_values(args.mask_path, args.sample_batch_size)
        if isinstance(paths, list):                                        # one mask per sample
            files = {f: load(f) for f in args.mask_path}
            known = torch.stack([files[f] for f in paths])
        else:
            known = load(paths)
        frames = trainer.inpaint(known, batch_size=args.sample_batch_size,
                        hard=not args.soft_mask, custom_t_list=sample_t_list, save_unbatched=True,
                        resample=args.resample, jump_length=args.jump_length, window=args.keep_window, **seed_kw)
    elif args.mode == 'outpaint':
        anchor = job_values(args.anchor, args.sample_batch_size)
        anchor = [tuple(a) for a in anchor] if isinstance(args.anchor, Jobs) else tuple(anchor)
        frames = trainer.outpaint(scale_mul, anchor=anchor, batch_size=args.sample_batch_size,
                         custom_t_list=sample_t_list, save_unbatched=True, resample=args.resample,
                         jump_length=args.jump_length, window=args.keep_window, **seed_kw)
    elif args.mode == 'paint2image':
        import numpy as np
        from PIL import Image
        h, w = ms_diffusion.target_size(n_scales - 1, scale_mul)

        def load(name):
            path = name if os.path.exists(name) else os.path.join(args.dataset_folder, name)
            pic = np.asarray(Image.open(path).convert("RGB").resize((w, h), Image.LANCZOS), dtype=np.float32)
            return torch.from_numpy(pic.transpose(2, 0, 1).copy()).div(255).mul(2).sub(1)

        names = job_values(args.input_image, args.sample_batch_size)
        if isinstance(names, list):                                        # one picture per sample
            files = {f: load(f) for f in args.input_image}
            layout = torch.stack([files[f] for f in names])
        else:
            layout = load(names)
        frames = trainer.paint2image(layout, batch_size=args.sample_batch_size, down=args.layout_down,
                            strength=job_values(args.layout_strength, args.sample_batch_size),
                            t_min=args.layout_t_min, scales=args.layout_scales, scale_mul=scale_mul,
                            custom_t_list=sample_t_list, save_unbatched=True, **seed_kw)
    elif args.mode == 'edit':
        import numpy as np
        from PIL import Image
        h, w = ms_diffusion.target_size(n_scales - 1, scale_mul)
        find = lambda name: name if os.path.exists(name) else os.path.join(args.dataset_folder, name)
        load_map = lambda f: torch.from_numpy(np.asarray(Image.open(find(f)).convert("L").resize((w, h), Image.BILINEAR),
                                                         dtype=np.float32).copy()).div(255)

        def load_pic(f):
            pic = np.asarray(Image.open(find(f)).convert("RGB").resize((w, h), Image.LANCZOS), dtype=np.float32)
            return torch.from_numpy(pic.transpose(2, 0, 1).copy()).div(255).mul(2).sub(1)

        def per_job(value, load):                                          # one tensor, or one per sample
            names = job_values(value, args.sample_batch_size)
            if not isinstance(names, list):
                return load(names)
            files = {f: load(f) for f in value}
            return torch.stack([files[f] for f in names])

        frames = trainer.edit(per_job(args.edit_map, load_map),
                              image=per_job(args.edit_image, load_pic) if args.edit_image else None,
                              batch_size=args.sample_batch_size, scale_mul=scale_mul, custom_t_list=sample_t_list,
                              save_unbatched=True, resample=args.resample, jump_length=args.jump_length,
                              window=args.keep_window, **seed_kw)
    elif args.mode == 'evaluate':
        if args.eval_scale is not None and args.eval_scale >= n_scales:
            raise SystemExit(f"--eval_scale {args.eval_scale} is past the {n_scales} scales")
        report = trainer.evaluate(batch_size=args.sample_batch_size, scale=args.eval_scale, patch=args.eval_patch,
                                  scale_mul=scale_mul, custom_sample=True, image_name=args.image_name,
                                  custom_t_list=sample_t_list, **refine_kw, **seed_kw)
        if rank == 0:
            for name in ("fidelity", "coherence", "coverage", "seam"):
                if name + "_mean" in report:
                    print(f"{name}: {report[name + '_mean']:.6g}")
            print("wrote " + os.path.join(results_folder, "patch_report.json"))
    elif args.mode == 'score':
        if args.score_scales is not None and args.score_scales[1] >= n_scales:
            raise SystemExit(f"--score_scales {args.score_scales} is past the {n_scales} scales")
        image = None
        if args.score_images is not None:
            import numpy as np
            from PIL import Image
            h, w = ms_diffusion.image_sizes[n_scales - 1]
            names = list(args.score_images) if isinstance(args.score_images, Jobs) else [args.score_images]

            def load(name):
                path = name if os.path.exists(name) else os.path.join(args.dataset_folder, name)
                pic = np.asarray(Image.open(path).convert("RGB").resize((w, h), Image.LANCZOS), dtype=np.float32)
                return torch.from_numpy(pic.transpose(2, 0, 1).copy()).div(255).mul(2).sub(1)

            image = torch.stack([load(f) for f in names])
        if args.seeds is not None and len(args.seeds) < args.score_draws:
            raise SystemExit(f"--mode score: {len(args.seeds)} seeds for --score_draws {args.score_draws} (one seed per draw)")
        report, _ = trainer.score(image=image, levels=args.score_levels, draws=args.score_draws, scales=args.score_scales,
                                  seeds=None if args.seeds is None else args.seeds[:args.score_draws])
        if rank == 0:
            for row in report["scales"]:
                print(f"scale {row['scale']}: " + "  ".join(f"{v:.6g}" for v in row["mean"]))
            print("wrote " + os.path.join(results_folder, "score_report.json"))
    else:
        raise NotImplementedError(
            f"mode {args.mode!r}: train, sample, style_transfer, harmonization, roi, inpaint, outpaint, paint2image, edit, evaluate and score are built for MI355X; "
            "the CLIP-guided modes of the reference need CLIP autograd and are out of scope (SURVEY.md section 8)")
    if args.gif is not None and frames and rank == 0:
        from sinddm_amd.functions import write_gif
        path = os.path.join(results_folder, f"{args.mode}_{'loop' if args.loop_seeds is not None else 'interp'}.gif")
        # (an interpolation plays once; a loop closes on itself: loop=0 repeats it for ever)
        write_gif(((frames[-1] + 1) * 0.5).clamp(0, 1).cpu(), path, args.gif, loop=0 if args.loop_seeds is not None else None)
        print("wrote " + path)
    if world > 1:
        td.destroy_process_group()


if __name__ == '__main__':
    main()
    quit()
