"""MultiscaleTrainer: training loop, multi-scale sampling driver, checkpoint I/O.

Mirror of reference SinDDM/trainer.py:35-285 (the hot-path part: __init__, train, sample_scales,
save, load, step_ema, reset_parameters, Dataset) and of its application drivers (image2image, roi_guided_sampling,
clip_sampling, clip_roi_sampling -- trainer.py:287-488; the two CLIP ones against any external scorer with the
reference's ClipExtractor interface: CLIP itself is not part of this build).
"""
from __future__ import annotations

import copy
import datetime
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch
from PIL import Image
from torch.optim.lr_scheduler import MultiStepLR

from . import dist as sdist
from .functions import num_to_groups
from .models import EMA, SinDDMNet
from .optim import FusedAdam, ema_update_


def image_to_tensor(img: Image.Image) -> torch.Tensor:
    """PIL RGB uint8 -> float32 CHW in [-1, 1]  (ToTensor + Lambda(t*2-1), trainer.py:46-50)."""
    a = np.asarray(img.convert('RGB'), dtype=np.uint8)
    return torch.from_numpy(a.transpose(2, 0, 1).copy()).to(torch.float32).div(255).mul(2).sub(1)


def image_to_tensor_01(img: Image.Image) -> torch.Tensor:
    """PIL RGB uint8 -> float32 CHW in [0, 1]  (torchvision ToTensor)."""
    a = np.asarray(img.convert('RGB'), dtype=np.uint8)
    return torch.from_numpy(a.transpose(2, 0, 1).copy()).to(torch.float32).div(255)


def save_image(tensor: torch.Tensor, path: str, nrow: int = 8, padding: int = 2) -> None:
    """Minimal stand-in for torchvision.utils.save_image (grid of [0,1] images -> PNG). Host side,
    off the timed path."""
    t = tensor.detach().float().cpu()
    if t.dim() == 3:
        t = t[None]
    t = t.clamp(0, 1)
    if t.shape[1] == 1:                      # (torchvision's make_grid shows a single-channel image as three equal channels)
        t = t.repeat(1, 3, 1, 1)
    B, C, H, W = t.shape
    if B == 1:
        # torchvision.utils.make_grid returns a single image as it is: no grid, no 2-pixel frame
        arr = t[0].mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
        Image.fromarray(arr).save(path)
        return
    ncol = min(nrow, B)
    nrows = (B + ncol - 1) // ncol
    grid = torch.zeros(C, nrows * (H + padding) + padding, ncol * (W + padding) + padding)
    for i in range(B):
        r, c = divmod(i, ncol)
        y, x = r * (H + padding) + padding, c * (W + padding) + padding
        grid[:, y:y + H, x:x + W] = t[i]
    arr = (grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy())
    Image.fromarray(arr).save(path)


class Dataset(torch.utils.data.Dataset):
    """One training image (and its blurry re-upsampled version) per scale folder (trainer.py:35-63)."""

    def __init__(self, folder, image_size, blurry_img=False, exts=('jpg', 'jpeg', 'png')):
        super().__init__()
        self.folder = folder
        self.image_size = image_size
        self.blurry_img = blurry_img
        self.paths = [p for ext in exts for p in Path(f'{folder}').glob(f'**/*.{ext}')]
        if blurry_img:
            self.folder_recon = folder + '_recon/'
            self.paths_recon = [p for ext in exts for p in Path(f'{self.folder_recon}').glob(f'**/*.{ext}')]

    def __len__(self):
        return len(self.paths) * 128

    def __getitem__(self, index):
        img = image_to_tensor(Image.open(self.paths[0]))
        if self.blurry_img:
            return img, image_to_tensor(Image.open(self.paths_recon[0]))
        return img


class MultiscaleTrainer(object):

    def __init__(self, ms_diffusion_model, folder, *, ema_decay=0.995, n_scales=None, scale_factor=1,
                 image_sizes=None, train_batch_size=32, train_lr=2e-5, train_num_steps=100000,
                 gradient_accumulate_every=2, fp16=False, step_start_ema=2000, update_ema_every=10,
                 save_and_sample_every=25000, avg_window=100, sched_milestones=None, results_folder='./results',
                 device=None, train_tile=(False, False), train_mask=None, train_mask_grow=0, train_mask_fill='mean',
                 train_crop=None, train_crop_margin=0):
        super().__init__()
        self.device = device
        self.sched_milestones = [10000, 30000, 60000, 80000, 90000] if sched_milestones is None else sched_milestones
        if image_sizes is None:
            image_sizes = []
        self.model = ms_diffusion_model
        self.ema = EMA(ema_decay)
        self.ema_decay = ema_decay
        self.ema_model = copy.deepcopy(self.model)
        # tileable training (wrap_y, wrap_x): the model that trains wraps its borders in p_losses.  The EMA copy never
        # trains; how it SAMPLES is its own `tile` setting.
        self.model.train_tile = (bool(train_tile[0]), bool(train_tile[1]))
        # crop training: (ch, cw) or None, and the margin the loss keeps from a window's open sides -- like `train_tile`, set
        # on the model that trains only (the EMA copy keeps None) and not stored in checkpoints.  train_step.TrainStep
        # refuses what does not fit (a crop with train_tile, a window within two margins) at the first step.
        self.model.train_crop = None if train_crop is None else (int(train_crop[0]), int(train_crop[1]))
        self.model.train_crop_margin = int(train_crop_margin)
        self.update_ema_every = update_ema_every
        self.step_start_ema = step_start_ema
        self.save_and_sample_every = save_and_sample_every
        self.avg_window = avg_window
        self.batch_size = train_batch_size
        self.n_scales = n_scales
        self.scale_factor = scale_factor
        self.gradient_accumulate_every = gradient_accumulate_every
        self.train_num_steps = train_num_steps

        # data-parallel training when launched under torch.distributed (one process per GPU): this rank trains on
        # its shard of the batch; gradients are summed with one all-reduce per optimizer step (sinddm_amd/dist.py)
        self.data_parallel = sdist.is_dist() and sdist.world_size() > 1
        self.local_batch_size = sdist.local_batch(train_batch_size) if self.data_parallel else train_batch_size
        if self.local_batch_size < 1:
            raise ValueError(f'train_batch_size={train_batch_size} leaves rank {sdist.rank()} without samples')
        self.loss_weight = self.local_batch_size / float(train_batch_size)
        self._scale_gen = None

        self.input_paths = []
        self.ds_list = []
        self.data_list = []
        self.results_folder = Path(results_folder)
        self.results_folder.mkdir(parents=True, exist_ok=True)

        # one batch of B identical copies per scale, parked on the device (trainer.py:113-132)
        for i in range(n_scales):
            self.input_paths.append(folder + 'scale_' + str(i))
            ds = Dataset(self.input_paths[i], image_sizes[i], blurry_img=i > 0)
            self.ds_list.append(ds)
            item = ds[0]
            rep = lambda t: t[None].repeat(self.local_batch_size, 1, 1, 1).contiguous().to(self.device)
            if i > 0:
                self.data_list.append((rep(item[0]), rep(item[1])))
            else:
                self.data_list.append((rep(item), rep(item)))

        # masked training: `train_mask` is an (H, W) {0,1} map at the finest size, 1 = train on this pixel.  The model that
        # trains gets one loss-weight map per scale (the hole grown by `train_mask_grow` pixels of each scale, across the
        # borders `train_tile` wraps), and with train_mask_fill = 'mean' the hole pixels of the training images -- the image
        # and its _recon partner -- are replaced by the mean of their valid pixels ('image' leaves them).  The EMA copy
        # never trains.  Every rank holds the same maps and normalises by its own B_local C sum(w); `loss_weight` does the rest.
        self.train_mask_hard = None
        if train_mask is not None:
            from .functions import fill_train_holes, keep_mask_pyramid, train_weight_pyramid
            if train_mask_fill not in ('mean', 'image'):
                raise ValueError(f"train_mask_fill {train_mask_fill!r} is neither 'mean' nor 'image'")
            sizes = [tuple(int(v) for v in self.model.image_sizes[i]) for i in range(n_scales)]      # (h, w) per scale
            valid = torch.as_tensor(train_mask).detach().to('cpu', torch.float32)
            if tuple(valid.shape) != sizes[-1]:
                raise ValueError(f'train_mask {tuple(valid.shape)} is not the finest scale {sizes[-1]}')
            weights = train_weight_pyramid(valid, sizes, grow=train_mask_grow, wrap=self.model.train_tile)
            self.train_mask_hard = [m.to(self.device) for m in keep_mask_pyramid(valid, sizes, hard=True)]
            self.model.train_weights = [w.to(self.device).contiguous() for w in weights]
            self.data_list = [tuple(fill_train_holes(img, self.train_mask_hard[i], train_mask_fill).contiguous()
                                    for img in pair) for i, pair in enumerate(self.data_list)]

        if fp16:
            raise NotImplementedError('apex mixed precision is never enabled by main.py (fp16=False, main.py:122)')
        self.fp16 = fp16

        if isinstance(self.model.denoise_fn, SinDDMNet):
            self.opt = FusedAdam(self.model.denoise_fn, lr=train_lr)
        else:
            self.opt = torch.optim.Adam(ms_diffusion_model.parameters(), lr=train_lr)
        self.scheduler = MultiStepLR(self.opt, milestones=self.sched_milestones, gamma=0.5)

        if self.data_parallel:
            # ranks seed their generators differently (own noise streams), so the initial weights must be agreed on
            with torch.no_grad():
                if isinstance(self.model.denoise_fn, SinDDMNet):
                    sdist.broadcast_(self.model.denoise_fn.flat_params)      # one 4.4 MB message
                    self.model.denoise_fn.mark_dirty()
                else:
                    for prm in self.model.denoise_fn.parameters():
                        sdist.broadcast_(prm.data)

        self.step = 0
        self.running_loss = []
        self.running_scale = []
        self.avg_t = []
        # optional injection hooks for parity tests: scale_fn(step) -> int
        self.scale_fn = None
        self.reset_parameters()

    def reset_parameters(self):
        """EMA weights := model weights (reference trainer.py:152-153).  The network's 52 tensors are one flat buffer: ONE
        launch (sinddm_adam_ema_step mode 2); the diffusion object's 13 schedule buffers are constants equal in both
        modules by construction, load_state_dict stays the path for foreign denoisers and CPU modules."""
        src, dst = self.model.denoise_fn, self.ema_model.denoise_fn
        if (isinstance(src, SinDDMNet) and isinstance(dst, SinDDMNet) and src.flat_params.is_cuda
                and dst.flat_params.is_cuda and src.flat_params.numel() == dst.flat_params.numel()):
            from .optim import ema_copy_
            ema_copy_(dst, src)
            return
        self.ema_model.load_state_dict(self.model.state_dict())

    def step_ema(self):
        """Copy until step_start_ema, then ema = decay*ema + (1-decay)*p  (trainer.py:155-159)."""
        if self.step < self.step_start_ema:
            self.reset_parameters()
            return
        src, dst = self.model.denoise_fn, self.ema_model.denoise_fn
        if isinstance(src, SinDDMNet) and isinstance(dst, SinDDMNet):
            ema_update_(dst, src, self.ema_decay)
        else:
            self.ema.update_model_average(self.ema_model, self.model)

    # ---- checkpoints: same file layout as the reference (trainer.py:161-187) so its model-N.pt files interoperate ----
    _CKPT_KEYS = ('step', 'model', 'ema', 'sched', 'running_loss', 'running_scale')

    def _ckpt_path(self, milestone) -> str:
        return str(self.results_folder / f'model-{milestone}.pt')

    def _checkpoint_state(self) -> dict:
        state = dict(zip(self._CKPT_KEYS, (self.step, self.model.state_dict(), self.ema_model.state_dict(),
                                           self.scheduler.state_dict(), self.running_loss, self.running_scale)))
        if isinstance(self.opt, FusedAdam):
            state['opt'] = self.opt.state_dict()       # extra key: the reference drops the Adam moments on save
        return state

    def _plot_running_loss(self) -> None:
        """running_loss.png next to the checkpoints (the reference plots the same curve); best effort, headless."""
        try:
            import matplotlib
            matplotlib.use('Agg')
            from matplotlib import pyplot as plt
        except Exception:
            return
        fig, ax = plt.subplots(figsize=(16, 8))
        ax.plot(self.running_loss)
        ax.set_ylim(0, 0.2)
        ax.grid(True)
        fig.savefig(str(self.results_folder / 'running_loss'))
        plt.close(fig)

    def save(self, milestone):
        torch.save(self._checkpoint_state(), self._ckpt_path(milestone))
        self._plot_running_loss()

    def load(self, milestone):
        state = torch.load(self._ckpt_path(milestone), map_location=self.device, weights_only=False)
        self.model.load_state_dict(state['model'])
        self.ema_model.load_state_dict(state['ema'])
        self.scheduler.load_state_dict(state['sched'])
        self.step, self.running_loss = state['step'], state['running_loss']
        if isinstance(self.opt, FusedAdam) and 'opt' in state:
            self.opt.load_state_dict(state['opt'])

    def _pick_scale(self, weights: torch.Tensor) -> int:
        if self.scale_fn is not None:
            return int(self.scale_fn(self.step))
        # trainer.py:197 (host draw: no sync); under data parallelism every rank draws from an identically
        # seeded private generator so that all ranks train the same scale in the same step
        return int(torch.multinomial(input=weights, num_samples=1, generator=self._scale_gen))

    def train(self):
        loss_acc = None
        s_weights = torch.tensor(self.model.num_timesteps_trained, dtype=torch.float)
        dp = self.data_parallel
        if dp and self._scale_gen is None:
            self._scale_gen = torch.Generator()
            # rank 0's seed, agreed on by broadcast; torch.initial_seed() only READS the global generator, so the
            # documented per-rank noise streams (manual_seed(1234 + rank) in main.py) stay what the user set
            self._scale_gen.manual_seed(sdist.broadcast_int(int(torch.initial_seed() % (2 ** 31))))
        net = self.model.denoise_fn
        while self.step < self.train_num_steps:
            s = self._pick_scale(s_weights)
            for _ in range(self.gradient_accumulate_every):
                data = self.data_list[s]
                self.model.crop_step = self.step                 # (what a crop_fn is called with)
                loss = self.model(data, s)
                if dp:
                    loss = loss * self.loss_weight       # shard mean -> this shard's share of the global-batch mean
                d = loss.detach()
                loss_acc = d if loss_acc is None else loss_acc + d
                (loss / self.gradient_accumulate_every).backward()
            if dp:
                # one collective per optimizer step on the flat gradient buffer (4.4 MB at dim=160)
                if isinstance(net, SinDDMNet):
                    sdist.allreduce_sum_(net.flat_grads)
                else:
                    for prm in self.model.parameters():
                        if prm.grad is not None:
                            sdist.allreduce_sum_(prm.grad)
            if self.step % self.avg_window == 0:
                if dp:
                    loss_acc = sdist.allreduce_sum_(loss_acc.reshape(1).clone())
                avg = float(loss_acc) / self.avg_window          # the only device->host sync of the loop
                if sdist.rank() == 0:
                    print(f'step:{self.step} loss:{avg}')
                self.running_loss.append(avg)
                loss_acc = None
            self.opt.step()
            self.opt.zero_grad()
            if self.step % self.update_ema_every == 0:
                self.step_ema()
            self.scheduler.step()
            self.step += 1
            if self.step % self.save_and_sample_every == 0 and sdist.rank() == 0:
                milestone = self.step // self.save_and_sample_every
                batches = num_to_groups(16, self.batch_size)
                all_images = torch.cat([self.ema_model.sample(batch_size=n) for n in batches], dim=0)
                all_images = (all_images + 1) * 0.5
                save_image(all_images, str(self.results_folder / f'sample-{milestone}.png'), nrow=4)
                self.save(milestone)
        if sdist.rank() == 0:
            print('training completed')

    @torch.no_grad()
    def sample_scales(self, scale_mul=None, batch_size=16, custom_sample=False, custom_image_size_idxs=None,
                      custom_scales=None, image_name='', start_noise=True, custom_t_list=None, desc=None,
                      save_unbatched=True, save_images=True, seeds=None, vary_from_scale=None,
                      seed_mix=None, patch_refine=None) -> List[torch.Tensor]:
        """Drive the sampler over all scales (behaviour of reference trainer.py:226-285).  Under torch.distributed the
        batch is sharded over ranks as independent chains and gathered with one all-gather per scale (RCCL over xGMI
        on MI355X); returns the list of per-scale (global) sample batches.
        `seeds`: the GLOBAL list of `batch_size` per-sample noise seeds (`ema_model.sample_seeds` for the duration of the
        call; a rank takes the seeds of its own shard, so the gathered batch holds the images a single process makes, in
        the same order).  `vary_from_scale` = S: scales >= S use seeds derived per sample (`models.vary_seeds`).
        Per-sample conditioning on `ema_model` (maps with a leading batch dimension, `layout_gain`, `roi_bbs_batch`) is GLOBAL
        too: `batch_size` rows, of which a rank takes its own shard's for the duration of the call (`dist.shard_rows`).
        `seed_mix`: in place of `seeds`, the GLOBAL blend tables (keys, weights), [batch_size][K] or
        [n_scales][batch_size][K] (`ema_model.seed_mix` for the duration of the call; `models.interp_seeds`, `loop_seeds`,
        `mix_from_scale`): sample b is frame b, and a rank takes the rows of its own shard like its seeds.
        `patch_refine`: a `refine.PatchRefine` or a dict of its fields (`iters`, `patch`, `alpha`, `blend`, `scales` = (a, b),
        `radius`).
        After the chain of every scale in [a, b] the rank's own shard is snapped to that scale's training image by `iters`
        field-and-vote iterations (`refine.patch_refine`; wrapped axes as `ema_model.tile`, holes of `train_mask` never
        copied from) before it is gathered and before the next scale upsamples it.  The iterations are independent per
        sample, so a sharded run makes the images of the single process.  With a `radius` only the first covered
        scale searches exhaustively: its last field, carried to the sizes of the next covered scale (`refine.carry_field`), is
        the prior of that scale's windowed search, and so on up the pyramid -- per sample as well.  With `keep_maps`,
        `layout_maps` or ROI guidance on `ema_model` it raises NotImplementedError (`sampler.NOT_BUILT`)."""
        em = self.ema_model
        if patch_refine is not None:
            from .refine import PatchRefine
            from .sampler import NOT_BUILT
            patch_refine = PatchRefine.of(patch_refine)
            for other, on in (('keep_maps', em.keep_maps is not None), ('layout_maps', em.layout_maps is not None),
                              ('roi', bool(em.roi_guided_sampling))):
                if on:
                    raise NotImplementedError(NOT_BUILT['patch_refine', other])
        options = self._call_options(seeds, vary_from_scale, seed_mix, batch_size, sharded=True)
        # --- what to run: one (scale, size index, start timestep) triple per stage ---
        scales = list(range(self.n_scales)) if custom_scales is None else list(custom_scales)
        size_idx = list(range(self.n_scales)) if custom_image_size_idxs is None else list(custom_image_size_idxs)
        t_starts = list(em.num_timesteps_ideal[1:]) if custom_t_list is None else list(custom_t_list)
        stretch = (1, 1) if scale_mul is None else scale_mul
        first_size = None
        if scale_mul is not None:
            h0, w0 = self.model.image_sizes[size_idx[0]]
            first_size = (int(h0 * scale_mul[0]), int(w0 * scale_mul[1]))
        # --- where the PNGs go (names as the reference writes them) ---
        tag = desc if desc is not None else f'sample_{str(datetime.datetime.now()).replace(":", "_")}'
        tag += '_rblr' if em.reblurring else ''
        tag += '_t_lmtd' if em.sample_limited_t else ''
        t_tag = '_'.join(str(e) for e in [em.num_timesteps_trained[0]] + t_starts)
        out_dir = Path(str(self.results_folder / 'final_samples'))
        writer = sdist.rank() == 0 and save_images
        if writer:
            out_dir.mkdir(parents=True, exist_ok=True)
        # --- this rank's chains ---
        if batch_size < sdist.world_size():
            raise ValueError(f'sample_scales: batch_size={batch_size} < world_size={sdist.world_size()} would leave ranks '
                             'without chains (every rank must join the all-gather)')
        mine = sdist.local_batch(batch_size)
        per_scale, cur, shown = [], None, None
        carried = None                                  # (field, sample size, image size) of the last refined scale
        with em.sampling(**options):
            for stage, s in enumerate(scales):
                if stage > 0:
                    cur = em.sample_via_scale(mine, cur, s=s, scale_mul=stretch, custom_sample=custom_sample,
                                              custom_img_size_idx=size_idx[stage], custom_t=t_starts[int(s) - 1])
                elif start_noise:
                    cur = em.sample(batch_size=mine, scale_0_size=first_size, s=s)
                else:                                   # start from the training image of that scale instead of noise
                    seed_img = Image.open(self.input_paths[s] + '/' + image_name).convert('RGB')
                    cur = image_to_tensor(seed_img).repeat(mine, 1, 1, 1).to(self.device)
                if patch_refine is not None and patch_refine.covers(s) and patch_refine.radius is not None:
                    from .refine import carry_field
                    sizes = (tuple(cur.shape[2:]), tuple(self.data_list[s][0][0].shape[1:]))
                    prior = None
                    if carried is not None:
                        prior = carry_field(carried[0], patch_refine.patch, carried[1], sizes[0], carried[2], sizes[1],
                                            wrap_query=tuple(em.tile))
                    cur, _, yx = self.refine(cur, scale=s, patch=patch_refine.patch, iters=patch_refine.iters,
                                             alpha=patch_refine.alpha, blend=patch_refine.blend, radius=patch_refine.radius,
                                             prior=prior, field=True)
                    carried = (yx,) + sizes
                elif patch_refine is not None and patch_refine.covers(s):
                    cur = self.refine(cur, scale=s, patch=patch_refine.patch, iters=patch_refine.iters,
                                      alpha=patch_refine.alpha, blend=patch_refine.blend)[0]
                whole = sdist.gather_batch(cur, batch_size)          # identity on a single process
                per_scale.append(whole)
                if writer:
                    shown = (whole + 1) * 0.5
                    save_image(shown, str(out_dir / t_tag) + f'_out_s{stage}_{tag}_sm_{stretch[0]}_{stretch[1]}.png', nrow=4)
        if writer and save_unbatched and shown is not None:
            single_dir = Path(str(self.results_folder / f'final_samples_unbatched_{tag}'))
            single_dir.mkdir(parents=True, exist_ok=True)
            for b, one in enumerate(shown):
                save_image(one, str(single_dir / t_tag) + f'_out_b{b}.png')
        return per_scale

    @torch.no_grad()
    def evaluate(self, samples=None, batch_size=16, scale=None, patch=7, **sample_kw) -> dict:
        """What the samples copy: the patch nearest-neighbour field (metrics.patch_report) between the batch of `scale`
        (default: the finest) and that scale's training image -- fidelity, coherence and coverage per sample, and `seam`
        when `ema_model.tile` wraps an axis.  Without `samples` (the list `sample_scales` returns) the batch is drawn here:
        `sample_scales(save_images=False, batch_size=batch_size, **sample_kw)`; a stretched sample (`scale_mul`) is simply
        compared at its own size.  A masked model (`train_mask`) is never scored against its hole.  Returns the report;
        rank 0 also writes it to `patch_report.json` in the results folder."""
        import json
        from .metrics import patch_report
        s = self.n_scales - 1 if scale is None else int(scale)
        if not 0 <= s < self.n_scales:
            raise ValueError(f'evaluate: scale {s} outside 0 ... {self.n_scales - 1}')
        if samples is None:
            samples = self.sample_scales(batch_size=batch_size, save_images=False, **sample_kw)
        batch = samples[s] if isinstance(samples, (list, tuple)) else samples
        image = self.data_list[s][0][0]
        valid = None if self.train_mask_hard is None else self.train_mask_hard[s]
        report = patch_report(batch.to(self.device, torch.float32).contiguous(), image.to(torch.float32).contiguous(),
                              patch=patch, tile=tuple(self.ema_model.tile), valid=valid)
        report['scale'] = s
        if sdist.rank() == 0:
            with open(str(self.results_folder / 'patch_report.json'), 'w') as f:
                json.dump(report, f, indent=1)
        return report

    @torch.no_grad()
    def refine(self, samples=None, scale=None, **kw):
        """Snap a batch to the training image's patches: `refine.patch_refine` of the batch of `scale` (default: the finest)
        against that scale's training image, with `ema_model.tile` as the wrapped axes and the hard `train_mask` as `valid`
        (a hole is never copied from).  `samples`: a batch, or the list `sample_scales` returns; without it a batch is drawn
        here (`batch_size`, default 16).  `kw` (`patch`, `iters`, `alpha`, `blend`, `weight`, `history`, `radius`, `prior`,
        `field`) goes to `patch_refine`, whose result is returned: (x, energy[, iterates][, yx])."""
        from .refine import patch_refine
        s = self.n_scales - 1 if scale is None else int(scale)
        if not 0 <= s < self.n_scales:
            raise ValueError(f'refine: scale {s} outside 0 ... {self.n_scales - 1}')
        batch_size = kw.pop('batch_size', 16)
        if samples is None:
            samples = self.sample_scales(batch_size=batch_size, save_images=False)
        batch = samples[s] if isinstance(samples, (list, tuple)) else samples
        image = self.data_list[s][0][0]
        valid = None if self.train_mask_hard is None else self.train_mask_hard[s]
        return patch_refine(batch.to(self.device, torch.float32).contiguous(), image.to(torch.float32).contiguous(),
                            tile=tuple(self.ema_model.tile), valid=valid, **kw)

    @torch.no_grad()
    def score(self, image=None, levels=10, draws=4, scales=None, seeds=None):
        """What the model thinks of a picture: the denoising score (`ema_model.denoise_score`, score.py) of the training
        pyramid and, with `image`, of that picture side by side with it.
            image   None: the checkpoint's own table -- per scale and per level, the loss of the trained weights on the images
                    they were trained on (`data_list`: each scale's picture and its blurred partner, the FILES of the pyramid).
                    (3,H,W) or (N,3,H,W) in [-1, 1] at the finest size: the picture(s) reach the scales through
                    score.score_pyramid (area averages; each blurred partner is the scale below, upsampled) and are scored in
                    one batch with the training image: row 0 is the training image, rows 1 ... N the pictures.
            levels  an int (that many levels per scale, score.score_levels over the levels the scale was trained on) or a list
            draws   noise draws per level (folded into the batch)
            scales  None (all) or (A, B), inclusive
            seeds   None, or `draws` ints in [0, 2^63): every row of every scale is scored under these same draws (common
                    random numbers: the picture and the training image differ by their content alone)
        The hard `train_mask` is the weight plane: a masked model is never scored against its hole, as in `evaluate`; the
        holes are exact zeros in every map, and the edit map's median and maximum are taken over the valid pixels only.
        Returns (report, maps): maps[s] is the (1 + N, H_s, W_s) score map of scale s; report holds, per scale, the levels, the
        per-level table and the mean of every row.  Every rank computes; rank 0 writes `score_report.json`, `score_s{S}.png`
        (the rows' maps over the training image's maximum) and, for a picture, `score_edit_map.png`: score.score_edit_map of
        the finest scored scale, a gray strength map that `--mode edit --edit_map` takes as it is (one per picture:
        `score_edit_map_{n}.png` from the second on).  No detection-rate claim is made."""
        import json
        from .score import score_edit_map, score_levels, score_pyramid
        em, n = self.ema_model, self.n_scales
        a, b = (0, n - 1) if scales is None else (int(scales[0]), int(scales[1]))
        if not 0 <= a <= b < n:
            raise ValueError(f'score: scales {(a, b)} outside 0 ... {n - 1}')
        draws = int(draws)
        if seeds is not None and len(seeds) != draws:
            raise ValueError(f'score: {len(seeds)} seeds for {draws} draws')
        sizes = [tuple(int(v) for v in em.image_sizes[s]) for s in range(n)]
        pics = None
        if image is not None:
            img = torch.as_tensor(image).to(torch.float32)
            if not bool(((img >= -1.0) & (img <= 1.0)).all()):
                raise ValueError('score: image outside [-1, 1]')
            pics = score_pyramid(img.to(self.device), sizes)
        report, maps = {'scales': [], 'draws': draws}, {}
        for s in range(a, b + 1):
            y = self.data_list[s][0][:1].to(torch.float32)
            yp = self.data_list[s][1][:1].to(torch.float32) if s > 0 else None
            if pics is not None:
                y = torch.cat([y, pics[s][0]])
                yp = torch.cat([yp, pics[s][1]]) if s > 0 else None
            lv = score_levels(em.num_timesteps_trained[s], levels) if isinstance(levels, int) else [int(t) for t in levels]
            weight = None if self.train_mask_hard is None else self.train_mask_hard[s].to(torch.float32).contiguous()
            rows = int(y.shape[0])
            row_seeds = None if seeds is None else [int(v) for _ in range(rows) for v in seeds]
            smap, table = em.denoise_score(y.contiguous(), s, y_prev=yp, levels=lv, draws=draws, seeds=row_seeds, weight=weight)
            maps[s] = smap
            report['scales'].append({'scale': s, 'size': list(sizes[s]), 'levels': lv,
                                     'table': table.t().cpu().tolist(),            # [row][level]
                                     'mean': table.mean(dim=0).cpu().tolist()})    # per row: row 0 = the training image
        if sdist.rank() == 0:
            with open(str(self.results_folder / 'score_report.json'), 'w') as f:
                json.dump(report, f, indent=1)
            for s, m in maps.items():
                top = m[0].max().clamp_min(1e-30)
                save_image((m / top)[:, None], str(self.results_folder / f'score_s{s}.png'), nrow=m.shape[0])
            if pics is not None:
                for k in range(1, maps[b].shape[0]):
                    # (under a train mask the holes of both maps are exact zeros: the normalisation leaves them out)
                    valid = None if self.train_mask_hard is None else self.train_mask_hard[b] > 0
                    em_map = score_edit_map(maps[b][k], maps[b][0], valid=valid).cpu()
                    arr = em_map.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).numpy()
                    name = 'score_edit_map.png' if k == 1 else f'score_edit_map_{k - 1}.png'
                    Image.fromarray(arr, mode='L').save(str(self.results_folder / name))
        return report, maps

    def _local_batch_maps(self, batch_size) -> dict:
        """This rank's rows of the per-sample conditioning on `ema_model`, as {attribute: value to set for the call}: every
        keep / layout map with a leading batch dimension, `layout_gain`, `roi_bbs_batch` and `roi_target_patch_batch` must have
        `batch_size` (global) rows and is cut with `dist.shard_rows`.  Empty when nothing is per sample."""
        em, B, out = self.ema_model, int(batch_size), {}

        def rows(v, what):
            n = int(v.shape[0]) if isinstance(v, torch.Tensor) else len(v)
            if n != B:
                raise ValueError(f'{what} has {n} rows for batch_size={B}')
            return sdist.shard_rows(v)

        if em.keep_maps is not None and any(m.dim() == 3 or k0.dim() == 4 for m, k0 in em.keep_maps.values()):
            out['keep_maps'] = {s: (rows(m, f'keep_maps[{s}] mask').contiguous() if m.dim() == 3 else m,
                                    rows(k0, f'keep_maps[{s}] x0').contiguous() if k0.dim() == 4 else k0)
                                for s, (m, k0) in em.keep_maps.items()}
        if em.layout_maps is not None and any(v.dim() == 4 for v in em.layout_maps.values()):
            out['layout_maps'] = {s: rows(v, f'layout_maps[{s}]').contiguous() if v.dim() == 4 else v
                                  for s, v in em.layout_maps.items()}
        for name in ('layout_gain', 'roi_bbs_batch', 'roi_target_patch_batch'):
            if getattr(em, name) is not None:
                out[name] = rows(getattr(em, name), name)
        return out

    def _local_seeds(self, seeds, vary_from_scale, batch_size, sharded):
        """`ema_model.sample_seeds` of a driver call: None without `seeds`; else the global list (checked against
        `batch_size`), expanded per scale when `vary_from_scale` is given, and -- for the drivers that shard the batch over
        ranks -- cut to this rank's samples.  The variation is derived from the GLOBAL position, before the cut."""
        from .models import _check_seed_row, vary_seeds
        if seeds is None:
            if vary_from_scale is not None:
                raise ValueError('vary_from_scale needs seeds')
            return None
        seeds = _check_seed_row(list(seeds), 'seeds')
        if len(seeds) != int(batch_size):
            raise ValueError(f'{len(seeds)} seeds for batch_size={int(batch_size)}')
        rows = [seeds] if vary_from_scale is None else vary_seeds(seeds, vary_from_scale, self.n_scales)
        if sharded:
            rows = [sdist.shard_seeds(r) for r in rows]
        return rows[0] if vary_from_scale is None else rows

    def _local_mix(self, seed_mix, seeds, batch_size, sharded):
        """`ema_model.seed_mix` of a driver call: None without `seed_mix`; else the global tables (checked against
        `batch_size`, every row validated) and -- for the drivers that shard the batch over ranks -- cut to this rank's rows
        with `dist.shard_rows`, before anything else reads them."""
        from .models import _check_mix
        if seed_mix is None:
            return None
        if seeds is not None:
            raise ValueError('seeds and seed_mix are both given: two noise sources')
        if not isinstance(seed_mix, (tuple, list)) or len(seed_mix) != 2:
            raise ValueError('seed_mix is a pair (keys, weights)')
        keys, w = (v.tolist() if isinstance(v, (np.ndarray, torch.Tensor)) else v for v in seed_mix)
        per_scale = len(keys) > 0 and len(keys[0]) > 0 and isinstance(keys[0][0], (list, tuple, np.ndarray, torch.Tensor))
        tabs = list(zip(keys, w)) if per_scale else [(keys, w)]
        if per_scale and (len(keys) != self.n_scales or len(w) != self.n_scales):
            raise ValueError(f'seed_mix has {len(keys)} / {len(w)} tables for {self.n_scales} scales')
        out = []
        for k, v in tabs:
            k, v = _check_mix(k, v)
            if len(k) != int(batch_size):
                raise ValueError(f'seed_mix holds {len(k)} rows for batch_size={int(batch_size)}')
            out.append((sdist.shard_rows(k), sdist.shard_rows(v)) if sharded else (k, v))
        if not per_scale:
            return out[0]
        return [k for k, _ in out], [v for _, v in out]

    def _call_options(self, seeds, vary_from_scale, seed_mix, batch_size, sharded) -> dict:
        """What a driver call hands `ema_model.sampling(...)`: `sample_seeds` / `seed_mix` when the call gives `seeds` /
        `seed_mix` (without them what `ema_model` carries stays in force) and, for the drivers that shard the batch over
        ranks, this rank's rows of the per-sample conditioning.  A key is there only when the call overrides it."""
        out = {'sample_seeds': self._local_seeds(seeds, vary_from_scale, batch_size, sharded),
               'seed_mix': self._local_mix(seed_mix, seeds, batch_size, sharded)}
        out = {k: v for k, v in out.items() if v is not None}
        if sharded:
            out.update(self._local_batch_maps(batch_size))
        return out

    # ---- application drivers of the reference that run entirely on the hot path ----
    def _i2i_source(self, input_folder, input_file, mask, hist_ref_path, image_name, use_hist, auto_scale, mode, device):
        """Host-side preparation of harmonization / style transfer: the (optionally shrunk, optionally histogram
        matched) source image as a [-1,1] tensor, and the blend mask (1 = keep the sample everywhere)."""
        import os
        from .functions import dilate_mask, match_histograms
        src = Image.open(os.path.join(input_folder, input_file)).convert("RGB")
        size = src.size
        if auto_scale is not None:
            shrink = np.sqrt((size[0] * size[1]) / auto_scale)
            if shrink > 1:
                size = (int(size[0] / shrink), int(size[1] / shrink))
                src = src.resize(size, Image.LANCZOS)
        keep = 1
        if mode == 'harmonization':
            m = Image.open(os.path.join(input_folder, mask)).convert("RGB").resize(size, Image.LANCZOS)
            keep = torch.from_numpy(dilate_mask(image_to_tensor_01(m), mode=mode)).to(device=device, dtype=torch.float32)
        if use_hist:
            ref = Image.open(hist_ref_path + image_name.rsplit(".", 1)[0] + '.png').convert("RGB")
            src = Image.fromarray(match_histograms(image=np.array(src), reference=np.array(ref), channel_axis=2))
        return image_to_tensor(src), keep

    @torch.no_grad()
    def image2image(self, input_folder='', input_file='', mask='', hist_ref_path='', image_name='', start_s=1,
                    custom_t=None, batch_size=16, scale_mul=(1, 1), device=None, use_hist=False, save_unbatched=True,
                    auto_scale=None, mode=None, save_images=True, seeds=None, vary_from_scale=None, seed_mix=None):
        """Harmonization / style transfer (behaviour of reference trainer.py:287-362): the input image is re-noised at
        scale `start_s` to `custom_t[start_s]` and denoised through the remaining scales by the trained model; in
        harmonization mode the result is pasted into the input through the dilated mask.  Returns the per-scale sample
        batches (the reference only writes PNGs).  `seeds` / `vary_from_scale` / `seed_mix`: as in `sample_scales` (this
        driver does not shard the batch: every process runs all `batch_size` chains)."""
        import os
        device = self.device if device is None else device
        em = self.ema_model
        options = self._call_options(seeds, vary_from_scale, seed_mix, batch_size, sharded=False)
        t_starts = em.num_timesteps_ideal if custom_t is None else custom_t
        src, keep = self._i2i_source(input_folder, input_file, mask, hist_ref_path, image_name, use_hist, auto_scale,
                                     mode, device)
        src_hw = torch.tensor(src.shape[1:])
        batch = src.repeat(batch_size, 1, 1, 1).to(device)
        if start_s > 0:
            # no blur mixing at the scale the chain starts from: its gamma row is zeroed in place, as the reference does
            em.gammas[start_s - 1].clamp_(0, 0)
        stamp = str(datetime.datetime.now()).replace(":", "_")
        t_tag = '_'.join(str(e) for e in t_starts)
        out_dir = Path(str(self.results_folder / 'i2i_final_samples'))
        if save_images:
            out_dir.mkdir(parents=True, exist_ok=True)
        last = self.n_scales - 1
        outs, shown = [], None
        with em.sampling(**options):
            for s in range(start_s, self.n_scales):
                # target size of this scale: the (possibly shrunk) input divided by scale_factor^(scales still to go)
                hw = src_hw / (self.scale_factor ** (last - s))
                target = (int(hw[0].item()), int(hw[1].item()))
                outs.append(em.sample_via_scale(batch_size, batch if not outs else outs[-1], s=s, custom_t=t_starts[s],
                                                scale_mul=scale_mul, custom_image_size=target))
                shown = (outs[-1] + 1) * 0.5
                if s == last:
                    shown = keep * shown + (1 - keep) * ((batch + 1) * 0.5).clamp_(0.0, 1.0)
                if save_images:
                    stem = input_file.rsplit(".", 1)[0]
                    save_image(shown, str(out_dir / f'{stem}_i2i_s_{s}_t_{t_tag}_hist_{"on" if use_hist else "off"}_{stamp}.png'),
                               nrow=4)
        if save_images and save_unbatched:
            single_dir = Path(str(self.results_folder / f'unbatched_i2i_s{start_s}_t_{t_tag}_{stamp}'))
            single_dir.mkdir(parents=True, exist_ok=True)
            for b in range(batch_size):
                save_image(shown[b], os.path.join(single_dir, input_file + f'_out_b{b}_i2i.png'))
        self.last_i2i_image = shown
        return outs

    @torch.no_grad()
    def roi_guided_sampling(self, custom_t_list=None, target_roi=None, roi_bb_list=None, save_unbatched=False,
                            batch_size=4, scale_mul=(1, 1), save_images=True, seeds=None, vary_from_scale=None,
                            per_sample=False, seed_mix=None):
        """ROI guided generation (trainer.py:436-454): at every scale but the finest the predicted clean image is
        pulled (eta = 0.8) towards a patch of the training image inside the given boxes; the blend runs inside the
        step kernels of the sampler's chain call (the edit maps of `sinddm_chain_opts`: one library call per scale,
        step noise from the in-kernel Philox stream).  With a `noise_fn`, or with `ema_model.chain_guided = False`,
        the run goes step by step through `sinddm_reverse_step_edit`.  `per_sample`: `roi_bb_list` holds `batch_size` box
        lists, one job per sample (`ema_model.roi_bbs_batch` -> the per-sample flags of `sinddm_batch_opts`); the target
        patch stays shared."""
        from .functions import extract_patch
        em = self.ema_model
        if per_sample and len(roi_bb_list) != int(batch_size):
            raise ValueError(f'roi_guided_sampling: {len(roi_bb_list)} box lists for batch_size={int(batch_size)}')
        boxes = [list(bbs) for bbs in roi_bb_list] if per_sample else None
        patches = []                   # (the reference appends on every call; a fresh list per call is what it means)
        for scale in range(self.n_scales):
            bb = [int(bb_i / np.power(self.scale_factor, self.n_scales - scale - 1)) for bb_i in target_roi]
            patches.append(extract_patch(self.data_list[scale][0][0][None, :, :, :], bb))
        # (the boxes and the patches stay on the model after the call, as in the reference)
        em.roi_bbs, em.roi_target_patch = [] if per_sample else roi_bb_list, patches
        with em.sampling(roi_guided_sampling=True, roi_bbs_batch=boxes):
            return self.sample_scales(scale_mul=scale_mul, custom_sample=False, image_name='', batch_size=batch_size,
                                      custom_t_list=custom_t_list,
                                      desc=f'roi_{str(datetime.datetime.now()).replace(":", "_")}',
                                      save_unbatched=save_unbatched, start_noise=True, save_images=save_images,
                                      seeds=seeds, vary_from_scale=vary_from_scale, seed_mix=seed_mix)

    # ---- known-region sampling: some pixels are given, the rest is generated to fit (no reference counterpart) ----
    def _sample_kept(self, keep_maps, tag, resample=1, jump_length=1, window=None, **kw):
        em = self.ema_model
        R, J = int(resample), int(jump_length)
        if R < 1 or J < 1:
            raise ValueError(f'{tag}: resample {resample} / jump_length {jump_length} must be >= 1')
        with em.sampling(keep_maps=keep_maps, resample=(R, J) if R > 1 else None, keep_window=window):
            return self.sample_scales(custom_sample=False, image_name='', start_noise=True,
                                      desc=f'{tag}_{str(datetime.datetime.now()).replace(":", "_")}', **kw)

    @torch.no_grad()
    def inpaint(self, mask, batch_size=16, hard=True, custom_t_list=None, save_unbatched=False, save_images=True,
                seeds=None, vary_from_scale=None, resample=1, jump_length=1, seed_mix=None, window=None):
        """Fill a hole in the training image: `mask` is (H, W) at the finest scale's size, 1 = keep the training image's
        pixel, 0 = generate.  At every scale the known image is that scale's training image and the mask comes from
        `functions.keep_mask_pyramid` (`hard`: a coarse pixel is kept only if its whole footprint is known); after every
        reverse step the known pixels are overwritten with the forward-diffused training image of that noise level, inside
        the step kernels (`ema_model.keep_maps` -> `sinddm_keep_opts` of the chain call: one library call per scale).
        `resample` = R > 1 adds RePaint's resampling: at every level that is a multiple of `jump_length` = J the run jumps
        back up by J levels and comes down again, until the stretch has been walked R times (`ema_model.resample` ->
        functions.resample_schedule and `sinddm_resample_opts`: still one library call per scale, R times the network
        evaluations on the resampled stretches).  The defaults (1, 1) are the run without jumps, bit for bit.  No
        image-quality claim is made.
        A (batch_size, H, W) stack of masks gives every sample its own hole: one job per sample, still one library call per
        scale (`sinddm_batch_opts`).
        `window` = None, or a margin in pixels (16, the network's receptive radius, makes it exact): at every scale the
        network then runs on each sample's window "bounding box of the pixels that may change, grown by the margin" only, with
        the draws of the full run (`ema_model.keep_window`, functions.keep_windows, sinddm_normal_fill_window): the run
        costs what its hole costs.  `outpaint` and `edit` take the same argument.
        Returns the per-scale batches and writes PNGs like `sample_scales`."""
        from .functions import keep_mask_pyramid
        em = self.ema_model
        m = torch.as_tensor(mask)
        fine = tuple(em.image_sizes[self.n_scales - 1])
        if tuple(m.shape) not in (fine, (int(batch_size),) + fine):
            raise ValueError(f'inpaint: mask {tuple(m.shape)} is not the finest scale {fine} (or {int(batch_size)} of them)')
        masks = keep_mask_pyramid(m, [em.image_sizes[s] for s in range(self.n_scales)], hard=hard, batch=m.dim() == 3)
        maps = {s: (masks[s].to(self.device).contiguous(), self.data_list[s][0][0].contiguous())
                for s in range(self.n_scales)}
        return self._sample_kept(maps, 'inpaint', resample=resample, jump_length=jump_length, batch_size=batch_size,
                                 custom_t_list=custom_t_list, save_unbatched=save_unbatched, save_images=save_images,
                                 seeds=seeds, vary_from_scale=vary_from_scale, seed_mix=seed_mix, window=window)

    @torch.no_grad()
    def outpaint(self, scale_mul, anchor=(0.5, 0.5), batch_size=16, custom_t_list=None, save_unbatched=False,
                 save_images=True, seeds=None, vary_from_scale=None, resample=1, jump_length=1, seed_mix=None, window=None):
        """Grow the canvas around the training image: at every scale the sample has `target_size(s, scale_mul)`, the
        scale's own training image sits unresampled at int(anchor * (canvas - image)) and is kept (mask 1 on that
        rectangle), the rest is generated.  `scale_mul` < 1 on an axis is a ValueError.  `resample` / `jump_length`: as for
        `inpaint`.  `anchor` may be a list of `batch_size` (y, x) pairs: every sample gets its own mask and known image."""
        from .functions import outpaint_offset
        em = self.ema_model
        if min(float(scale_mul[0]), float(scale_mul[1])) < 1:
            raise ValueError(f'outpaint: scale_mul {tuple(scale_mul)} < 1 would crop the known image')
        anchors = None
        if len(anchor) > 0 and isinstance(anchor[0], (tuple, list)):
            anchors = [tuple(a) for a in anchor]
            if len(anchors) != int(batch_size):
                raise ValueError(f'outpaint: {len(anchors)} anchors for batch_size={int(batch_size)}')
        maps = {}
        for s in range(self.n_scales):
            img = self.data_list[s][0][0]
            h, w = int(img.shape[1]), int(img.shape[2])
            Hc, Wc = em.target_size(s, scale_mul)
            pairs = []
            for a in (anchors if anchors is not None else [anchor]):
                y0, x0 = outpaint_offset((Hc, Wc), (h, w), a)
                k0 = torch.zeros((img.shape[0], Hc, Wc), dtype=torch.float32, device=img.device)
                m = torch.zeros((Hc, Wc), dtype=torch.float32, device=img.device)
                k0[:, y0:y0 + h, x0:x0 + w] = img
                m[y0:y0 + h, x0:x0 + w] = 1.0
                pairs.append((m, k0))
            maps[s] = pairs[0] if anchors is None else (torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs]))
        return self._sample_kept(maps, 'outpaint', resample=resample, jump_length=jump_length, scale_mul=tuple(scale_mul),
                                 batch_size=batch_size,
                                 custom_t_list=custom_t_list, save_unbatched=save_unbatched, save_images=save_images,
                                 seeds=seeds, vary_from_scale=vary_from_scale, seed_mix=seed_mix, window=window)

    # ---- per-pixel edit strength: every pixel its own SDEdit start level (no reference counterpart) ----
    @torch.no_grad()
    def edit(self, strength, image=None, batch_size=16, scale_mul=(1, 1), custom_t_list=None, seeds=None,
             vary_from_scale=None, seed_mix=None, resample=1, jump_length=1, save_unbatched=False, save_images=True,
             window=None):
        """Edit a picture with a strength per pixel: `strength` is (H, W) in [0, 1] at the finest target size
        (`ema_model.target_size(n_scales - 1, scale_mul)`), 0 = leave the pixel alone, 1 = redraw it from scratch, c in
        between = re-noise it to the share c of the scale's levels and let the model take it from there (SDEdit with a start
        level per pixel).  `image` is the (3, H, W) picture in [-1, 1] being edited; None: the training image of every scale
        (`data_list`, as `inpaint` uses it; `scale_mul` must then be (1, 1)).  The picture reaches the scales by area averaging
        (`functions._layout_pyramid`), the strength as the hold level 1 - strength (`functions.hold_pyramid`).  At every
        scale a reverse step that lands on level u keeps -- overwrites with the forward-diffused picture of level u, as
        `inpaint` does -- the pixels with strength <= (u + 1) / (t_top + 1) and leaves the others to the model
        (`ema_model.keep_maps` + `keep_gated` -> `sinddm_gate_opts` of the chain call: still one library call per scale).  A
        {0, 1} map is `inpaint(1 - strength)` bit for bit.  `resample` / `jump_length`: as for `inpaint` (after a jump back up
        a released pixel is pinned again until the run is back at its level).  No image-quality claim is made.
        `strength` may be (batch_size, H, W) and `image` (batch_size, 3, H, W): one job per sample (`sinddm_batch_opts`).
        Returns the per-scale batches and writes PNGs like `sample_scales`."""
        from .functions import _layout_pyramid, hold_pyramid
        em, B = self.ema_model, int(batch_size)
        st = torch.as_tensor(strength)
        sizes = [tuple(em.target_size(s, scale_mul)) for s in range(self.n_scales)]
        fine = sizes[-1]
        if tuple(st.shape) not in (fine, (B,) + fine):
            raise ValueError(f'edit: strength {tuple(st.shape)} is not the finest target size {fine} (or {B} of them)')
        st = st.to(torch.float32)
        if not bool(((st >= 0.0) & (st <= 1.0)).all()):
            raise ValueError('edit: strength outside [0, 1]')
        if image is None:
            if tuple(float(v) for v in scale_mul) != (1.0, 1.0):
                raise ValueError(f'edit: scale_mul {tuple(scale_mul)} needs an image (the training pyramid has its own sizes)')
            known = [self.data_list[s][0][0].contiguous() for s in range(self.n_scales)]
        else:
            img = torch.as_tensor(image)
            if tuple(img.shape) not in ((3,) + fine, (B, 3) + fine):
                raise ValueError(f'edit: image {tuple(img.shape)} must be (3, {fine[0]}, {fine[1]}), the finest target size, '
                                 f'or {B} of them')
            img = img.to(torch.float32)
            if not bool(((img >= -1.0) & (img <= 1.0)).all()):
                raise ValueError('edit: image outside [-1, 1]')
            known = [k.to(self.device).contiguous() for k in _layout_pyramid(img, sizes)]
        holds = hold_pyramid(st, sizes, batch=st.dim() == 3)
        maps = {s: (holds[s].to(self.device).contiguous(), known[s]) for s in range(self.n_scales)}
        # ((1, 1) goes in as `inpaint` hands it over: no scale_mul)
        sm = {} if tuple(float(v) for v in scale_mul) == (1.0, 1.0) else {'scale_mul': tuple(scale_mul)}
        with em.sampling(keep_gated=True):
            return self._sample_kept(maps, 'edit', resample=resample, jump_length=jump_length, **sm, batch_size=batch_size,
                                     custom_t_list=custom_t_list, save_unbatched=save_unbatched, save_images=save_images,
                                     seeds=seeds, vary_from_scale=vary_from_scale, seed_mix=seed_mix, window=window)

    # ---- layout conditioning: redraw a rough picture in the training image's texture (no reference counterpart) ----
    @torch.no_grad()
    def paint2image(self, layout, batch_size=16, down=8, strength=1.0, t_min=0, scales=None, scale_mul=(1, 1), seeds=None,
                    vary_from_scale=None, custom_t_list=None, save_unbatched=False, save_images=True, seed_mix=None):
        """Paint-to-image: `layout` is a (3, H, W) picture in [-1, 1] at the finest target size
        (`ema_model.target_size(n_scales - 1, scale_mul)`) -- a scribble, a colour sketch, a blurred photo, another sample.
        At every reverse step with t >= `t_min` the low spatial frequencies of the predicted clean image are pulled towards
        the layout's with `strength` in [0, 1]; the high frequencies stay the model's own.  "Low" is the band below `down`
        pixels at the finest scale, the same physical band at every scale (`functions.layout_blocks`); the layout reaches
        each scale by area averaging (`functions._layout_pyramid`).  `scales` = (first, last) limits the conditioned scales
        (inclusive; default all).  Runs `sample_scales` with `ema_model.layout_maps` / `layout_down` / `layout_strength` /
        `layout_t_min` set for the call (`sinddm_layout_opts` of the chain call: still one library call per scale).
        strength = 0 is `sample_scales` itself, bit for bit.  No image-quality claim is made.
        `layout` may be (batch_size, 3, H, W), one picture per sample, and `strength` a list of `batch_size` values: their
        maximum becomes the shared per-step strength and value / maximum the sample's `layout_gain`
        (`split_strength`; `sinddm_batch_opts::layout_gain`)."""
        from .functions import layout_blocks, _layout_pyramid, split_strength
        em = self.ema_model
        lay = torch.as_tensor(layout)
        sizes = [tuple(em.target_size(s, scale_mul)) for s in range(self.n_scales)]
        if tuple(lay.shape) not in ((3,) + sizes[-1], (int(batch_size), 3) + sizes[-1]):
            raise ValueError(f'paint2image: layout {tuple(lay.shape)} must be (3, {sizes[-1][0]}, {sizes[-1][1]}), the finest '
                             f'target size, or {int(batch_size)} of them')
        strength, gain = split_strength(strength, batch_size)
        if not (0.0 <= float(strength) <= 1.0) or int(t_min) < 0:
            raise ValueError(f'paint2image: strength {strength} outside [0, 1] or t_min {t_min} < 0')
        first, last = (0, self.n_scales - 1) if scales is None else (int(scales[0]), int(scales[1]))
        if not 0 <= first <= last < self.n_scales:
            raise ValueError(f'paint2image: scales {scales} outside 0 ... {self.n_scales - 1}')
        blocks = layout_blocks(down, self.scale_factor, self.n_scales)
        pyr = _layout_pyramid(lay.to(torch.float32), sizes)
        maps = {s: pyr[s].to(self.device).contiguous() for s in range(first, last + 1)}
        with em.sampling(layout_maps=maps, layout_down={s: blocks[s] for s in range(first, last + 1)},
                         layout_strength=float(strength), layout_t_min=int(t_min), layout_gain=gain):
            return self.sample_scales(scale_mul=tuple(scale_mul), custom_sample=False, image_name='', start_noise=True,
                                      desc=f'paint2image_{str(datetime.datetime.now()).replace(":", "_")}',
                                      batch_size=batch_size, custom_t_list=custom_t_list, save_unbatched=save_unbatched,
                                      save_images=save_images, seeds=seeds, vary_from_scale=vary_from_scale,
                                      seed_mix=seed_mix)

    # ---- CLIP-driven modes of the reference.  CLIP itself (clip/, text2live_util/) is not part of this build; the
    # driver takes any `clip_model` with the interface the reference uses: get_text_embedding(text, template=...),
    # zero_grad(), calculate_clip_loss(image in [0,1], embedding) (differentiable), cfg["n_aug"] ----
    def clip_sampling(self, clip_model, text_input, strength, sample_batch_size, custom_t_list=None,
                      guidance_sub_iters=None, quantile=0.8, stop_guidance=None, save_unbatched=False, scale_mul=(1, 1),
                      llambda=0, start_noise=True, image_name='', templates=('hr', 'lr')):   # trainer.py:363-410
        em = self.ema_model
        if guidance_sub_iters is None:
            guidance_sub_iters = [*reversed(range(self.n_scales))]
        embedds_hr = clip_model.get_text_embedding(text_input, template=templates[0])
        embedds_lr = clip_model.get_text_embedding(text_input, template=templates[1])
        n_aug = getattr(clip_model, "cfg", {}).get("n_aug", 0)
        desc = (f"clip_{text_input.replace(' ', '_')}_n_aug{n_aug}_str_{strength}_gsi_" + '_'.join(str(e) for e in guidance_sub_iters)
                + f'_ff{1 - quantile}' + f'_{str(datetime.datetime.now()).replace(":", "_")}')
        # (the CLIP state stays on the model after the call, as in the reference)
        em.clip_strength = strength
        em.clip_text = text_input
        em.text_embedds_hr, em.text_embedds_lr = embedds_hr, embedds_lr
        em.guidance_sub_iters = guidance_sub_iters
        em.quantile = quantile
        em.stop_guidance = stop_guidance
        em.clip_model = clip_model
        em.clip_score = []
        em.llambda = llambda
        em.clip_mask = None
        em.x_recon_prev = None
        with em.sampling(clip_guided_sampling=True):
            if not start_noise:                                            # clip_style_trans: start from the last two scales
                return self.sample_scales(scale_mul=scale_mul, custom_sample=True,
                                          custom_scales=[self.n_scales - 2, self.n_scales - 1],
                                          custom_image_size_idxs=[self.n_scales - 2, self.n_scales - 1],
                                          image_name=image_name, batch_size=sample_batch_size, custom_t_list=custom_t_list,
                                          desc=desc, save_unbatched=save_unbatched, start_noise=start_noise)
            return self.sample_scales(scale_mul=scale_mul, custom_sample=False, image_name='', batch_size=sample_batch_size,
                                      custom_t_list=custom_t_list, desc=desc, save_unbatched=save_unbatched,
                                      start_noise=start_noise)

    def clip_roi_sampling(self, clip_model, text_input, strength, sample_batch_size, num_clip_iters=100,
                          num_denoising_steps=2, clip_roi_bb=None, save_unbatched=False, template='lr',
                          save_images=True):                                      # trainer.py:412-468
        """Text-guided edit of a region of the training image: `num_clip_iters` steps of normalised gradient ascent of
        the external score on the ROI alone (step = strength * |roi| / |grad| per sample, clamped to [-1, 1] -- plain
        autograd on the ROI tensor, no network involved), the patch pasted back into the image, then the finest
        scale's sampler for `num_denoising_steps` reverse steps (q_sample to t = num_denoising_steps + the HIP chain) to
        blend it in.  Returns the final batch in [-1, 1]."""
        em = self.ema_model
        y0, x0, h, w = clip_roi_bb
        top = self.n_scales - 1
        emb = clip_model.get_text_embedding(text_input, template=template)
        image = self.data_list[top][0][0][None].repeat(sample_batch_size, 1, 1, 1).clone()
        roi = image[:, :, y0:y0 + h, x0:x0 + w].clone()
        trace_dir = Path(str(em.results_folder / 'interm_samples_clip_roi'))
        if em.save_interm:
            trace_dir.mkdir(parents=True, exist_ok=True)
        norm = lambda v: torch.linalg.vector_norm(v, dim=(1, 2, 3), keepdim=True)
        for it in range(num_clip_iters):
            roi = roi.detach().requires_grad_(True)
            clip_model.zero_grad()
            with torch.enable_grad():
                score = -clip_model.calculate_clip_loss((roi + 1) * 0.5, emb)
                grad = torch.autograd.grad(score, roi, create_graph=False)[0]
            if em.save_interm:
                save_image((roi.detach().clamp(-1., 1.) + 1) * 0.5, str(trace_dir / f'iter_{it}.png'), nrow=4)
            with torch.no_grad():
                roi = (roi + strength * (norm(roi) / norm(grad)) * grad).clamp_(-1., 1.)
        image[:, :, y0:y0 + h, x0:x0 + w] = roi.detach()
        final = em.sample_via_scale(sample_batch_size, image, s=top, custom_t=num_denoising_steps, scale_mul=(1, 1))
        if save_images:
            n_aug = getattr(clip_model, "cfg", {}).get("n_aug", 0)
            tag = (f"clip_roi_{text_input.replace(' ', '_')}_n_aug{n_aug}_str_{strength}_n_iters_{num_clip_iters}"
                   f'_{str(datetime.datetime.now()).replace(":", "_")}')
            shown = (final + 1) * 0.5
            out_dir = Path(str(em.results_folder / 'final_samples'))
            out_dir.mkdir(parents=True, exist_ok=True)
            save_image(shown, str(out_dir / (tag + '.png')), nrow=4)
            if save_unbatched:
                single_dir = Path(str(self.results_folder / f'final_samples_unbatched_{tag}'))
                single_dir.mkdir(parents=True, exist_ok=True)
                for b in range(sample_batch_size):
                    save_image(shown[b], str(single_dir / f'{tag}_out_b{b}.png'))
        return final
