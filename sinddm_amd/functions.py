"""Host-side helpers of the SinDDM hot path (mirror of reference SinDDM/functions.py:72-192).

Everything here is one-off host work (schedule maths in float64 numpy, pyramid construction with
PIL) or tiny glue; the per-step work lives in the HIP library.
"""
from __future__ import annotations

from inspect import isfunction
from pathlib import Path
from typing import List, Sequence, Tuple

import numpy as np
import torch
from PIL import Image


def exists(x) -> bool:                                   # functions.py:72
    return x is not None


def default(val, d):                                     # functions.py:76
    if exists(val):
        return val
    return d() if isfunction(d) else d


def cycle(dl):                                           # functions.py:82
    while True:
        for data in dl:
            yield data


def num_to_groups(num: int, divisor: int) -> List[int]:  # functions.py:88
    groups, remainder = divmod(num, divisor)
    arr = [divisor] * groups
    if remainder > 0:
        arr.append(remainder)
    return arr


def loss_backwards(fp16, loss, optimizer, **kwargs):     # functions.py:97 (apex AMP is never enabled)
    if fp16:
        raise NotImplementedError("apex mixed precision is not part of the MI355X build (fp16=False in main.py:122)")
    loss.backward(**kwargs)


def extract(a: torch.Tensor, t: torch.Tensor, x_shape) -> torch.Tensor:
    """a[t] reshaped (B,1,1,1) -- functions.py:105-108.  Kept for API parity; the HIP kernels do
    this gather themselves (table pointer + t)."""
    b = t.shape[0]
    return a.gather(-1, t).reshape(b, *((1,) * (len(x_shape) - 1)))


def noise_like(shape, device, repeat: bool = False) -> torch.Tensor:   # functions.py:111-114
    if repeat:
        return torch.randn((1, *shape[1:]), device=device).repeat(shape[0], *((1,) * (len(shape) - 1)))
    return torch.randn(shape, device=device)


def cosine_beta_schedule(timesteps: int, s: float = 0.008) -> np.ndarray:
    """Cosine schedule in float64 (functions.py:117-127)."""
    steps = timesteps + 1
    grid = np.linspace(0, steps, steps)
    abar = np.cos(((grid / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    abar = abar / abar[0]
    betas = 1 - (abar[1:] / abar[:-1])
    return np.clip(betas, a_min=0, a_max=0.999)


def pyramid_geometry(image_size: Tuple[int, int], scale_factor: float = 1.411, auto_scale=None):
    """Integer / float64 bookkeeping of create_img_scales (functions.py:148-174): returns
    (sizes[(W,H)], scale_factor, n_scales, image_size_used).  No image data involved."""
    image_size = (int(image_size[0]), int(image_size[1]))
    if auto_scale is not None:
        scaler = np.sqrt((image_size[0] * image_size[1]) / auto_scale)
        if scaler > 1:
            image_size = (int(image_size[0] / scaler), int(image_size[1] / scaler))
    area_scale_0 = 3110
    s_dim, l_dim = min(image_size), max(image_size)
    scale_0_dim = int(round(np.sqrt(area_scale_0 * s_dim / l_dim)))
    scale_0_dim = min(max(scale_0_dim, 42), 55)
    n_scales = int(round((np.log(s_dim / scale_0_dim)) / (np.log(scale_factor))) + 1)
    scale_factor = np.exp((np.log(s_dim / scale_0_dim)) / (n_scales - 1))
    sizes = []
    for i in range(n_scales):
        f = np.power(scale_factor, n_scales - i - 1)
        sizes.append((int(round(image_size[0] / f)), int(round(image_size[1] / f))))
    return sizes, scale_factor, n_scales, image_size


def create_img_scales(foldername, filename, scale_factor=1.411, image_size=None, create=False, auto_scale=None):
    """Build the image pyramid of one training image (functions.py:130-192).

    LANCZOS down-scales into <folder>/scale_i/, BILINEAR re-upsamples of scale i-1 into
    <folder>/scale_i_recon/, and the wrapped-uint8 Frobenius 'rescale loss' per scale.
    Returns (sizes[(W,H)], rescale_losses, scale_factor, n_scales) exactly like the reference."""
    orig_image = Image.open(foldername + filename)
    filename = filename.rsplit(".", 1)[0] + ".png"
    if image_size is None:
        image_size = orig_image.size
    sizes, scale_factor, n_scales, _ = pyramid_geometry(image_size, scale_factor, auto_scale)

    pyramid = []
    for i, size in enumerate(sizes):
        img = orig_image.resize(size, Image.LANCZOS)
        if create:
            out_dir = Path(foldername + f"scale_{i}/")
            out_dir.mkdir(parents=True, exist_ok=True)
            img.save(str(out_dir / filename))
        pyramid.append(img)

    rescale_losses = []
    for i in range(n_scales - 1):
        recon = pyramid[i].resize(sizes[i + 1], Image.BILINEAR)
        # uint8 subtraction wraps around, as in the reference (np.subtract on PIL images)
        diff = np.subtract(pyramid[i + 1], recon)
        rescale_losses.append(np.linalg.norm(diff) / np.asarray(recon).size)
        if create:
            out_dir = Path(foldername + f"scale_{i + 1}_recon/")
            out_dir.mkdir(parents=True, exist_ok=True)
            recon.save(str(out_dir / filename))
    return sizes, rescale_losses, scale_factor, n_scales


# ---- helpers of the application drivers (reference SinDDM/functions.py:21-48) ----------------------------
def extract_patch(image: torch.Tensor, bb) -> torch.Tensor:              # functions.py:45-48
    y_bb, x_bb, h_bb, w_bb = bb
    return image[:, :, y_bb:y_bb + h_bb, x_bb:x_bb + w_bb]


def stat_from_bbs(image: torch.Tensor, bb):                              # functions.py:38-42
    y_bb, x_bb, h_bb, w_bb = bb
    reg = image[:, :, y_bb:y_bb + h_bb, x_bb:x_bb + w_bb]
    return [torch.mean(reg, dim=(2, 3), keepdim=True), torch.std(reg, dim=(2, 3), keepdim=True)]


# ---- helpers of known-region sampling (MultiscaleTrainer.inpaint / outpaint; no reference counterpart) --------------
def _area_weights(n_out: int, n_in: int) -> np.ndarray:
    """(n_out, n_in) float64: row i holds the share of input pixel j in output pixel i's footprint [i r, (i + 1) r),
    r = n_in / n_out.  The overlaps are integers in units of 1 / n_out, so a pixel is in the footprint or not -- no
    rounding decides it -- and every row sums to 1."""
    i = np.arange(n_out, dtype=np.int64)[:, None]
    j = np.arange(n_in, dtype=np.int64)[None, :]
    overlap = np.minimum((i + 1) * n_in, (j + 1) * n_out) - np.maximum(i * n_in, j * n_out)
    return np.maximum(overlap, 0).astype(np.float64) / float(n_in)


def keep_mask_pyramid(mask, sizes, hard: bool = True, batch: bool = False) -> List[torch.Tensor]:
    """A full-resolution {0,1} mask (H, W), 1 = known, brought to every scale by area averaging: one fp32 (h, w) tensor
    per entry of `sizes` ((h, w) pairs), on the mask's device.  `hard` keeps a pixel only if its whole footprint is known
    (average >= 1 - 1e-6; the smallest share of a footprint pixel is 1 / H): a coarse pixel that mixes known and unknown
    content is generated, never pinned.  hard=False returns the averages (the step kernels blend with them).
    `batch`: the mask is a (B, H, W) stack, one job per sample, and the tensors are (B, h, w): row b is what the call returns
    for mask b alone.  It has to be asked for: a 3-d mask handed over by mistake (an RGB picture) stays an error."""
    m = torch.as_tensor(mask)
    if batch:
        if m.dim() != 3 or m.shape[0] < 1:
            raise ValueError(f"keep_mask_pyramid: a batch of masks must be (B, H, W), got {tuple(m.shape)}")
        rows = [keep_mask_pyramid(m[b], sizes, hard) for b in range(m.shape[0])]
        return [torch.stack([r[i] for r in rows]) for i in range(len(rows[0]))]
    if m.dim() != 2:
        raise ValueError(f"keep_mask_pyramid: mask must be (H, W), got {tuple(m.shape)}")
    device = m.device
    full = m.detach().to("cpu", torch.float64).numpy()
    out = []
    for h, w in sizes:
        h, w = int(h), int(w)
        if h > full.shape[0] or w > full.shape[1]:
            raise ValueError(f"keep_mask_pyramid: scale {(h, w)} is larger than the mask {full.shape}")
        avg = _area_weights(h, full.shape[0]) @ full @ _area_weights(w, full.shape[1]).T
        if hard:
            avg = (avg >= 1.0 - 1e-6).astype(np.float64)
        out.append(torch.from_numpy(np.clip(avg, 0.0, 1.0).astype(np.float32)).to(device))
    return out


# ---- helpers of per-pixel edit strength (MultiscaleTrainer.edit; no reference counterpart) ---------------------------
def gate_thresholds(lands: Sequence[int], t_top: int) -> np.ndarray:
    """The per-step thresholds of a level-gated keep run (sinddm_gate_opts), their ONE owner: for a step that lands on level
    `land` (-1: the clean image) of a run whose highest level is `t_top`,
        thr = 1 - (land + 1) / (t_top + 1)
    evaluated in float64 and stored as fp32.  A pixel of hold level h = 1 - strength is kept by the step iff h >= thr, i.e.
    iff strength <= (land + 1) / (t_top + 1): strength 0 is kept through to the clean image (thr = 1 exactly on landing
    clean), strength 1 is never kept (thr > 0 always), strength c is released when the run has c (t_top + 1) levels left.
    The rule reads the landing level alone, so strided schedules and resampling jumps need nothing special: after a jump
    back up a released pixel is pinned again until the run comes back down to its level.  Every land must lie in
    [-1, t_top - 1], which keeps every threshold inside (0, 1]."""
    top = int(t_top)
    u = np.asarray([int(v) for v in lands], dtype=np.int64)
    if top < 0 or (u.size and (int(u.min()) < -1 or int(u.max()) > top - 1)):
        raise ValueError(f"gate_thresholds: lands {u.tolist()} outside [-1, t_top - 1] for t_top = {t_top}")
    thr = (1.0 - (u.astype(np.float64) + 1.0) / float(top + 1)).astype(np.float32)
    assert bool(np.all((thr > 0.0) & (thr <= 1.0)))
    return thr


def hold_pyramid(strength, sizes, batch: bool = False) -> List[torch.Tensor]:
    """A finest-size strength map (H, W) in [0, 1] (0 = keep the known image, 1 = redraw freely) brought to every (h, w) of
    `sizes` by area averaging, returned as the HOLD LEVEL 1 - strength the gated keep reads: one fp32 (h, w) tensor per scale
    on the map's device.  The footprints are `_area_weights`' with the division done last (the overlaps are integers in
    units of 1 / n_out), so a constant map stays constant and a {0, 1} map on regions that are whole footprints stays {0, 1},
    exactly.  `batch`: a (B, H, W) stack, one job per sample, gives (B, h, w) tensors: row b is what the call returns for map
    b alone (it has to be asked for, as in `keep_mask_pyramid`)."""
    m = torch.as_tensor(strength)
    if batch:
        if m.dim() != 3 or m.shape[0] < 1:
            raise ValueError(f"hold_pyramid: a batch of strength maps must be (B, H, W), got {tuple(m.shape)}")
        rows = [hold_pyramid(m[b], sizes) for b in range(m.shape[0])]
        return [torch.stack([r[i] for r in rows]) for i in range(len(rows[0]))]
    if m.dim() != 2:
        raise ValueError(f"hold_pyramid: strength must be (H, W), got {tuple(m.shape)}")
    device = m.device
    full = m.detach().to("cpu", torch.float64).numpy()
    if not bool(np.all((full >= 0.0) & (full <= 1.0))):                     # (a NaN fails both)
        raise ValueError("hold_pyramid: strength outside [0, 1]")
    H, W = full.shape
    out = []
    for h, w in sizes:
        h, w = int(h), int(w)
        if h > H or w > W or h < 1 or w < 1:
            raise ValueError(f"hold_pyramid: scale {(h, w)} does not fit the strength map {full.shape}")
        # (weights * n_in are the integer overlaps: sums of a {0, 1} map are exact, and a whole footprint gives H * W)
        num = np.rint(_area_weights(h, H) * H) @ full @ np.rint(_area_weights(w, W) * W).T
        avg = num / (float(H) * float(W))
        out.append(torch.from_numpy(np.clip(1.0 - avg, 0.0, 1.0).astype(np.float32)).to(device))
    return out


# ---- helpers of masked training (MultiScaleGaussianDiffusion.train_weights; no reference counterpart) ----------------
def _grow_1d(hole: np.ndarray, g: int, axis: int, wrap: bool) -> np.ndarray:
    """Boolean dilation of `hole` by `g` pixels to both sides along `axis`: across the border, modulo the size, with `wrap`;
    stopping at it otherwise.  A windowed sum over the padded array: exact integer arithmetic."""
    n = hole.shape[axis]
    if g == 0:
        return hole
    g = min(g, n)                                        # g >= n covers the whole axis either way
    pad = [(0, 0), (0, 0)]
    pad[axis] = (g, g)
    padded = np.pad(hole.astype(np.int64), pad, mode="wrap" if wrap else "constant")
    c = np.cumsum(padded, axis=axis)
    zero = np.zeros_like(np.take(c, [0], axis=axis))
    c = np.concatenate([zero, c], axis=axis)
    return (np.take(c, np.arange(2 * g + 1, 2 * g + 1 + n), axis=axis) - np.take(c, np.arange(0, n), axis=axis)) > 0


def train_weight_pyramid(valid, sizes, grow=0, wrap=(False, False)) -> List[torch.Tensor]:
    """The loss weights of masked training, one fp32 {0,1} (h, w) map per entry of `sizes`, on the device of `valid`.
    `valid` is an (H, W) {0,1} map at the finest size, 1 = train on this pixel.  Each scale's map is
    keep_mask_pyramid(hard=True) -- a coarse pixel whose footprint touches the hole is out -- with the hole then dilated by
    `grow` pixels OF THAT SCALE (an int, or one value per scale) by a square structuring element: the network's receptive
    field is a square of Chebyshev radius 16 (SINDDM_TILE_HALO), so with grow = 16 no pixel that trains has a hole pixel in
    view, and the weights provably never see what the hole contains.  On an axis of `wrap` = (wrap_y, wrap_x) -- the
    `train_tile` of the run -- the hole grows across the border, modulo the size; otherwise it stops there.
    ValueError: a negative grow, a list of another length than `sizes`, a mask that is not (H, W), a scale left without a
    valid pixel (named: coarse scales may not survive a large grow -- give one value per scale)."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    grows = [int(grow)] * len(sizes) if np.ndim(grow) == 0 else [int(g) for g in grow]
    if len(grows) != len(sizes):
        raise ValueError(f"train_weight_pyramid: {len(grows)} grow values for {len(sizes)} scales (give one, or one per scale)")
    if any(g < 0 for g in grows):
        raise ValueError(f"train_weight_pyramid: grow {grows} must be >= 0")
    m = torch.as_tensor(valid)
    if m.dim() != 2:
        raise ValueError(f"train_weight_pyramid: the mask must be (H, W), got {tuple(m.shape)}")
    out = []
    for s, (hard, g) in enumerate(zip(keep_mask_pyramid(m, sizes, hard=True), grows)):
        hole = hard.cpu().numpy() < 0.5
        hole = _grow_1d(_grow_1d(hole, g, 0, bool(wrap[0])), g, 1, bool(wrap[1]))
        if bool(hole.all()):
            raise ValueError(f"train_weight_pyramid: scale {s} {sizes[s]} has no valid pixel left with grow = {g}")
        out.append(torch.from_numpy((~hole).astype(np.float32)).to(m.device))
    return out


def fill_train_holes(img: torch.Tensor, hard_valid: torch.Tensor, fill: str = "mean") -> torch.Tensor:
    """A copy of the (..., C, h, w) image(s) `img` of one scale with the hole pixels (`hard_valid` (h, w) == 0: the UN-grown
    hard mask of the scale) replaced: fill = 'mean' writes the per-channel mean of the image's valid pixels (float64,
    rounded to the image's dtype), so that what the network sees inside the hole is flat instead of the damage; 'image'
    leaves the picture as it is.  The valid pixels are returned bit for bit."""
    if fill not in ("mean", "image"):
        raise ValueError(f"fill_train_holes: fill {fill!r} is neither 'mean' nor 'image'")
    v = torch.as_tensor(hard_valid).to(img.device) > 0.5
    if img.dim() < 3 or tuple(v.shape) != tuple(img.shape[-2:]):
        raise ValueError(f"fill_train_holes: mask {tuple(v.shape)} against an image {tuple(img.shape)}")
    if fill == "image" or bool(v.all()):
        return img.clone()
    if not bool(v.any()):
        raise ValueError("fill_train_holes: no valid pixel to take the mean of")
    img64 = img.to(torch.float64)
    mean = torch.where(v, img64, torch.zeros_like(img64)).sum(dim=(-2, -1), keepdim=True) / float(v.sum())
    return torch.where(v, img, mean.to(img.dtype).expand_as(img))


# ---- helpers of crop training (MultiScaleGaussianDiffusion.train_crop; no reference counterpart) ----------
def crop_window(size, crop) -> Tuple[int, int]:
    """The window (h, w) = (min(ch, H), min(cw, W)) of a scale of `size` = (H, W) under `crop` = (ch, cw)."""
    return min(int(crop[0]), int(size[0])), min(int(crop[1]), int(size[1]))


def crop_windows(gen, B: int, size, crop, margin: int) -> torch.Tensor:
    """The clamped draw: a CPU int64 (B, 2) table of window origins (y0, x0).  Per cropped axis (window h < size H), with
    L = h - 2 margin: o' uniform over the integers -(L-1) .. H - h + (L-1) from the torch.Generator `gen`, y0 = clamp(o', 0,
    H - h); an axis the window spans gets 0.  Every pixel of the axis then lies in the valid range (`crop_rects`) of at least
    L and at most 3 L of the H - h + 2 L - 1 draws, where a uniform y0 would leave a border pixel to a single one.
    ValueError: L < 1 on a cropped axis."""
    cols = []
    for n, k in zip(size, crop_window(size, crop)):
        n = int(n)
        if k == n:
            cols.append(torch.zeros(int(B), dtype=torch.int64))
            continue
        L = k - 2 * int(margin)
        if L < 1:
            raise ValueError(f"crop_windows: a window of {k} leaves nothing inside a margin of {margin}")
        o = torch.randint(-(L - 1), n - k + (L - 1) + 1, (int(B),), generator=gen, dtype=torch.int64)
        cols.append(o.clamp_(0, n - k))
    return torch.stack(cols, dim=1)


def crop_rects(windows, size, crop, margin: int) -> torch.Tensor:
    """The valid rectangles of `windows` ((B, 2) origins), in window coordinates: a CPU int64 (B, 4) table (y_lo, y_hi, x_lo,
    x_hi), half open.  A side of a window that lies on the image border is closed and keeps its pixels; every other side is
    open and loses `margin` rows or columns (the network's zero padding lies there)."""
    win = torch.as_tensor(windows).detach().to("cpu", torch.int64).reshape(-1, 2)
    m, cols = int(margin), []
    for axis, (n, k) in enumerate(zip(size, crop_window(size, crop))):
        o = win[:, axis]
        cols += [torch.where(o == 0, 0, m), torch.where(o == int(n) - k, k, k - m)]
    return torch.stack(cols, dim=1)


def summed_area_table(w: torch.Tensor) -> torch.Tensor:
    """The float64 (H + 1, W + 1) summed-area table of an (H, W) map, on the CPU: sat[y, x] = sum of w[:y, :x]."""
    w64 = torch.as_tensor(w).detach().to("cpu", torch.float64)
    sat = torch.zeros(w64.shape[0] + 1, w64.shape[1] + 1, dtype=torch.float64)
    sat[1:, 1:] = w64.cumsum(0).cumsum(1)
    return sat


def crop_norm(windows, rects, sat=None) -> float:
    """sum over the samples of the total weight of their valid rectangles -- what a cropped step divides by, times C.
    Without a map (`sat` None) it is area arithmetic; with one, `sat` is `summed_area_table(map)` and every sample costs four
    look-ups at the full-image corners of its rectangle.  Host integers and float64: no device work."""
    win = torch.as_tensor(windows).detach().to("cpu", torch.int64).reshape(-1, 2)
    r = torch.as_tensor(rects).detach().to("cpu", torch.int64).reshape(-1, 4)
    hh, ww = (r[:, 1] - r[:, 0]).clamp_(min=0), (r[:, 3] - r[:, 2]).clamp_(min=0)
    if sat is None:
        return float(int((hh * ww).sum()))
    y0, x0 = win[:, 0] + r[:, 0], win[:, 1] + r[:, 2]
    y1, x1 = y0 + hh, x0 + ww
    tot = sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]
    return float(torch.where((hh * ww) > 0, tot, torch.zeros_like(tot)).sum())


# ---- the window of a known-region run (MultiScaleGaussianDiffusion.keep_window; no reference counterpart) ----
def keep_windows(free, margin: int = 16, batch=None):
    """The windows a known-region run has to compute: `free` is a bool (H, W) or (B, H, W) map, True where the pixel is not held
    for the whole run (mask < 1 under `keep_maps`, hold level < 1 under `keep_gated`).  Per sample the bounding box of the free
    pixels is grown by `margin` on every side and clipped to the image; the common size (h, w) is the largest such box, w
    rounded up to a multiple of 4 where that is still <= W (the cropped rows stay on the step tails' 16-byte path); sample b's
    origin is (min(y0_b, H - h), min(x0_b, W - w)), so that its grown box lies inside its window; a sample without a free
    pixel gets (0, 0).  Returns None when no sample has a free pixel or when (h, w) == (H, W) -- the run is then the full
    run -- else (h, w, origins), origins an int32 CPU (B, 2) tensor; a shared (H, W) map gives one origin, replicated
    `batch` times (once without `batch`).  With margin >= 16, the network's receptive radius (_lib.TILE_HALO), the free pixels
    of the windowed run are the full run's.  SinddmError: `margin` not an integer >= 0."""
    from ._lib import SinddmError
    if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)) or int(margin) < 0:
        raise SinddmError(f"keep_windows: margin {margin!r} is not an integer >= 0")
    g = int(margin)
    f = torch.as_tensor(free).detach().to("cpu")
    if f.dim() not in (2, 3):
        raise SinddmError(f"keep_windows: free map {tuple(f.shape)} is neither (H, W) nor (B, H, W)")
    shared = f.dim() == 2
    f = (f[None] if shared else f) != 0
    H, W = int(f.shape[1]), int(f.shape[2])
    boxes = []                                              # per sample (y0, y1, x0, x1) of the grown box, or None
    for fb in f:
        rows, cols = torch.nonzero(fb.any(dim=1)).reshape(-1), torch.nonzero(fb.any(dim=0)).reshape(-1)
        if rows.numel() == 0:
            boxes.append(None)
            continue
        boxes.append((max(int(rows[0]) - g, 0), min(int(rows[-1]) + 1 + g, H), max(int(cols[0]) - g, 0),
                      min(int(cols[-1]) + 1 + g, W)))
    live = [b for b in boxes if b is not None]
    if not live:
        return None
    h, w = max(b[1] - b[0] for b in live), max(b[3] - b[2] for b in live)
    if -(-w // 4) * 4 <= W:
        w = -(-w // 4) * 4
    if (h, w) == (H, W):
        return None
    origins = torch.tensor([(0, 0) if b is None else (min(b[0], H - h), min(b[2], W - w)) for b in boxes], dtype=torch.int32)
    if shared:
        origins = origins.repeat(int(batch) if batch is not None else 1, 1)
    return h, w, origins


def outpaint_offset(canvas, image, anchor=(0.5, 0.5)) -> Tuple[int, int]:
    """Top-left corner (y, x) of an (h, w) image placed on an (H, W) canvas: int(anchor * (canvas - image)) per axis;
    anchor (0, 0) = top left, (0.5, 0.5) = centred, (1, 1) = bottom right."""
    for a, big, small in zip(anchor, canvas, image):
        if not 0.0 <= float(a) <= 1.0:
            raise ValueError(f"outpaint: anchor {tuple(anchor)} outside [0, 1]")
        if int(big) < int(small):
            raise ValueError(f"outpaint: canvas {tuple(canvas)} smaller than the image {tuple(image)} (scale_mul < 1)")
    return int(float(anchor[0]) * (int(canvas[0]) - int(image[0]))), int(float(anchor[1]) * (int(canvas[1]) - int(image[1])))


def resample_schedule(t_seq: Sequence[int], resample: int = 1, jump: int = 1):
    """The walk of a resampled run (RePaint's resampling on this sampler's level convention), its ONE owner.  `t_seq` is the
    descending run of reverse steps `_run_steps` gets (step t takes a state at noise level t and writes one at level t - 1);
    L = t_seq[0] is its input level.  Walk down; after a step that reaches level l a jump back up to l + J follows when
    l >= 0, l % J == 0, l + J <= L and that anchor has been jumped from fewer than R - 1 times; the walk goes on with step
    t = l + J.  Anchors do not nest (the levels l + J - 1 .. l + 1 are no multiples of J), so the number of steps is
    len(t_seq) + (R - 1) * J * |anchors|.  t_seq = 9..0, J = 3, R = 2:  9 8 7 ^9 9 8 7 6 5 4 ^6 6 5 4 3 2 1 ^3 3 2 1 0.
    Returns (steps, jump_to): the expanded step list and, per step, the level to jump to afterwards or None.  R = 1 returns
    t_seq with no jumps."""
    steps = [int(t) for t in t_seq]
    R, J = int(resample), int(jump)
    if R < 1 or J < 1:
        raise ValueError(f"resample_schedule: resample {resample} / jump {jump} must be >= 1")
    if R == 1 or not steps:
        return steps, [None] * len(steps)
    if steps[-1] < 0 or any(a - b != 1 for a, b in zip(steps, steps[1:])):
        raise ValueError("resample_schedule: t_seq must descend in steps of 1 and stay >= 0")
    L, t_min = steps[0], steps[-1]
    out, jump_to, used = [], [], {}
    t = L
    while t >= t_min:
        lvl = t - 1
        out.append(t)
        if lvl >= 0 and lvl % J == 0 and lvl + J <= L and used.get(lvl, 0) < R - 1:
            used[lvl] = used.get(lvl, 0) + 1
            jump_to.append(lvl + J)
            t = lvl + J
        else:
            jump_to.append(None)
            t = lvl
    return out, jump_to


# ---- few-step sampling (no reference counterpart: the reference evaluates the network at every level) ----------------
def stride_schedule(t_seq: Sequence[int], n: int, spacing: str = "t", kappa=None):
    """The levels of a few-step run, its ONE owner.  `t_seq` is the descending run [a, a-1, ..., b] `_run_steps` gets; at most
    `n` of its levels are kept.  Returns (taus, lands): the network is evaluated at taus[i] and that step lands on level
    lands[i] = taus[i + 1]; the last step lands on b - 1 (-1: the clean image).  taus[0] = a, and taus[-1] = b when more than
    one level is kept.
      spacing 't'       rint(linspace(a, b, min(n, len(t_seq))))
      spacing 'logsnr'  for each of n equally spaced values of log kappa between levels a and b, the level of the run nearest
                        in log kappa; `kappa[l]` (float64, indexed by level) must rise strictly as l falls over the run
    Both drop duplicates, so fewer than n levels may remain.  n >= len(t_seq) returns t_seq itself with lands = t - 1."""
    steps = [int(t) for t in t_seq]
    n = int(n)
    if n < 1:
        raise ValueError(f"stride_schedule: n = {n} must be >= 1")
    if spacing not in ("t", "logsnr"):
        raise ValueError(f"stride_schedule: spacing {spacing!r} is neither 't' nor 'logsnr'")
    if not steps:
        return [], []
    if steps[-1] < 0 or any(a - b != 1 for a, b in zip(steps, steps[1:])):
        raise ValueError("stride_schedule: t_seq must descend in steps of 1 and stay >= 0")
    a, b = steps[0], steps[-1]
    if spacing == "logsnr":
        if kappa is None:
            raise ValueError("stride_schedule: spacing 'logsnr' needs kappa")
        kap = np.asarray(kappa, dtype=np.float64)[b:a + 1]                  # kap[j]: level b + j
        if kap.shape[0] != len(steps) or not bool(np.all(np.isfinite(kap)) and np.all(kap > 0.0) and np.all(np.diff(kap) < 0.0)):
            raise ValueError("stride_schedule: kappa must be finite, positive and rise strictly as the level falls over the run")
    if n >= len(steps):
        return steps, [t - 1 for t in steps]
    if spacing == "t":
        taus = [int(v) for v in np.rint(np.linspace(a, b, n))]
    else:
        lam = np.log(kap)
        taus = [b + int(np.argmin(np.abs(lam - v))) for v in np.linspace(lam[-1], lam[0], n)]
        taus[0] = a
        if n > 1:
            taus[-1] = b
    taus = sorted(set(taus), reverse=True)
    return taus, taus[1:] + [b - 1]


# ---- helpers of layout conditioning (MultiscaleTrainer.paint2image; no reference counterpart) ------------------------
def layout_strengths(t_seq: Sequence[int], strength: float = 1.0, t_min: int = 0) -> List[float]:
    """The per-step strengths g_i of a layout-conditioned run: `strength` at the steps with t >= t_min, 0 below (those steps
    keep their fused tail: the last, least noisy steps are left to the model).  `strength` must lie in [0, 1]."""
    g = float(strength)
    if not 0.0 <= g <= 1.0:
        raise ValueError(f"layout_strengths: strength {strength} outside [0, 1]")
    if int(t_min) < 0:
        raise ValueError(f"layout_strengths: t_min {t_min} must be >= 0")
    return [g if int(t) >= int(t_min) else 0.0 for t in t_seq]


def split_strength(strength, batch_size: int):
    """`strength` of paint2image -> (shared per-step strength, per-sample gains or None).  One number: (it, None).  A
    sequence of `batch_size` values in [0, 1]: their maximum in fp32 and value / maximum per sample (fp32; all ones when the
    maximum is 0), so that the step's strength for sample b, the fp32 product, is the sample's own value to one rounding."""
    if np.ndim(strength) == 0:
        return float(strength), None
    v = np.asarray(strength, dtype=np.float32).reshape(-1)
    if v.shape[0] != int(batch_size):
        raise ValueError(f"paint2image: {v.shape[0]} strengths for batch_size={int(batch_size)}")
    if not bool(np.all((v >= 0.0) & (v <= 1.0))):
        raise ValueError(f"paint2image: strength {v.tolist()} outside [0, 1]")
    top = np.float32(v.max())
    gain = v / top if top > 0 else np.ones_like(v)
    return float(top), [float(x) for x in gain]


def layout_blocks(n_finest: int, scale_factor: float, n_scales: int) -> List[int]:
    """Block size per scale for a block of `n_finest` pixels at the finest one: N_s = max(1, round(N / f^(n_scales-1-s))),
    the same physical band at every scale.  1 <= n_finest <= 64 (the kernels' range)."""
    n = int(n_finest)
    if not 1 <= n <= 64:
        raise ValueError(f"layout_blocks: block size {n_finest} outside 1 ... 64")
    if int(n_scales) < 1 or not float(scale_factor) > 1.0:
        raise ValueError(f"layout_blocks: n_scales {n_scales} / scale_factor {scale_factor}")
    return [max(1, int(round(n / float(scale_factor) ** (int(n_scales) - 1 - s)))) for s in range(int(n_scales))]


def _layout_pyramid(layout, sizes) -> List[torch.Tensor]:
    """A (3, H, W) layout picture brought to every (h, w) of `sizes` by area averaging (`_area_weights`: every output
    pixel is a convex combination, so a constant image stays constant and the range is kept): fp32 tensors on the layout's
    device.  A (B, 3, H, W) stack of pictures gives (B, 3, h, w) tensors: row b is what the call returns for picture b alone."""
    lay = torch.as_tensor(layout)
    if lay.dim() == 4 and lay.shape[0] > 0 and lay.shape[1] == 3:
        rows = [_layout_pyramid(lay[b], sizes) for b in range(lay.shape[0])]
        return [torch.stack([r[i] for r in rows]) for i in range(len(rows[0]))]
    if lay.dim() != 3 or lay.shape[0] != 3:
        raise ValueError(f"_layout_pyramid: layout must be (3, H, W) or (B, 3, H, W), got {tuple(lay.shape)}")
    device = lay.device
    full = lay.detach().to("cpu", torch.float64).numpy()
    out = []
    for h, w in sizes:
        h, w = int(h), int(w)
        if h > full.shape[1] or w > full.shape[2] or h < 1 or w < 1:
            raise ValueError(f"_layout_pyramid: scale {(h, w)} does not fit the layout {full.shape[1:]}")
        avg = np.einsum("ij,cjk,lk->cil", _area_weights(h, full.shape[1]), full, _area_weights(w, full.shape[2]))
        out.append(torch.from_numpy(avg.astype(np.float32)).to(device))
    return out


def write_gif(frames, path, ms: int, loop=0) -> str:
    """The (N, 3, H, W) batch `frames` (values in [0, 1]) as one animated GIF at `path`, frame b shown for `ms` milliseconds
    in batch order.  `loop` = 0 repeats for ever (a closed loop of `loop_seeds`), None plays once."""
    arr = torch.as_tensor(frames).detach().to("cpu", torch.float32)
    if arr.dim() != 4 or arr.shape[1] != 3 or arr.shape[0] < 1:
        raise ValueError(f"write_gif: frames must be (N, 3, H, W), got {tuple(arr.shape)}")
    if int(ms) < 1:
        raise ValueError(f"write_gif: {ms} ms per frame")
    pics = [Image.fromarray((f.clamp(0, 1).mul(255).add(0.5).to(torch.uint8).permute(1, 2, 0).numpy())) for f in arr]
    kw = {} if loop is None else {"loop": int(loop)}
    pics[0].save(str(path), format="GIF", save_all=True, append_images=pics[1:], duration=int(ms), disposal=1, **kw)
    return str(path)


def _disk(radius: int) -> np.ndarray:
    """skimage.morphology.disk: (2r+1)^2 footprint of the pixels within Euclidean distance r."""
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    return (xx * xx + yy * yy) <= radius * radius


def dilate_mask(mask: torch.Tensor, mode: str) -> np.ndarray:
    """functions.py:21-33 -- binary dilation by a disk (radius 7 harmonization / 20 editing), Gaussian blur
    (sigma 5), min-max normalisation; returns (1,1,H,W).  The reference calls scikit-image (pinned 0.19.3; absent from this
    image's Python): restated on scipy.ndimage with scikit-image's defaults (binary_dilation: border value False;
    filters.gaussian: mode='nearest', truncate=4.0, float64) and PINNED by fixture G20 = the reference's lines run on
    scikit-image 0.18.3 itself (tests/golden/make_golden_skimage.py; agreement < 1e-12, tests/test_host.py)."""
    from scipy import ndimage as ndi
    if mode == "harmonization":
        element = _disk(7)
    elif mode == "editing":
        element = _disk(20)
    else:
        raise ValueError(mode)
    m = np.asarray(mask.permute(1, 2, 0)[:, :, 0]) != 0
    m = ndi.binary_dilation(m, structure=element)
    m = ndi.gaussian_filter(m.astype(np.float64), sigma=5, mode="nearest", truncate=4.0)
    m = m[None, None, :, :]
    return (m - m.min()) / (m.max() - m.min())


def match_histograms(image: np.ndarray, reference: np.ndarray, channel_axis: int = 2) -> np.ndarray:
    """skimage.exposure.match_histograms (0.19.3) for uint8 HxWxC images, as used by image2image
    (trainer.py:312-314): per channel, map every source level through the reference's inverse CDF
    (np.interp of the cumulative histograms) and store into the input dtype.  Pinned bit for bit by fixture G20 (scikit-image
    0.18.3's own output, tests/golden/make_golden_skimage.py)."""
    if image.ndim != reference.ndim or channel_axis != image.ndim - 1:
        raise ValueError("expects HxWxC arrays with the channel axis last")
    if image.shape[-1] != reference.shape[-1]:
        raise ValueError("Number of channels in the input image and reference image must match!")
    out = np.empty(image.shape, dtype=image.dtype)
    for ch in range(image.shape[-1]):
        src, tmpl = image[..., ch], reference[..., ch]
        lookup = src.reshape(-1)
        src_counts = np.bincount(lookup)
        tmpl_counts = np.bincount(tmpl.reshape(-1))
        tmpl_values = np.nonzero(tmpl_counts)[0]
        tmpl_counts = tmpl_counts[tmpl_values]
        src_q = np.cumsum(src_counts) / src.size
        tmpl_q = np.cumsum(tmpl_counts) / tmpl.size
        interp = np.interp(src_q, tmpl_q, tmpl_values)
        out[..., ch] = interp[lookup].reshape(src.shape)
    return out


def thresholded_grad(grad, quantile=0.8):
    """Soft-thresholded guidance gradient + the mask of the positions that survive (reference SinDDM/functions.py:52-67):
    per sample the pixel-wise gradient energy ||grad||_2 over channels is reduced by its `quantile` (nearest) and clamped
    at 0; the direction of the gradient is kept.  Returns (sparse_grad (B,C,H,W), mask (B,1,H,W) bool)."""
    energy = torch.norm(grad, dim=1)                                                   # (B,H,W)
    q = torch.quantile(energy.reshape(energy.shape[0], -1), q=quantile, dim=1, interpolation='nearest')[:, None, None]
    excess = energy - q
    mask = (excess > 0)[:, None, :, :]
    unit = grad / energy[:, None, :, :]
    unit[torch.isnan(unit)] = 0
    return torch.clamp(excess, min=0)[:, None, :, :] * unit, mask
