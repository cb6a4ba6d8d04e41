"""float64 numpy restatement of layout conditioning, written from the definitions in include/sinddm_hip.h (the contract), not
from the kernels: the clean estimate xp, the block delta D, the upsampled delta U and the conditioned reverse step.

Shapes: images are (..., H, W) arrays over the BUFFER size H x W = (Hc + 2 halo_y) x (Wc + 2 halo_x); D is (..., h, w) with
h = ceil(Hc / N), w = ceil(Wc / N).  An axis with a halo wraps; `wrap` adds the flag of the halo-less step-by-step route.
"""
import numpy as np


def coefs(k):
    """The fields of a StepCoefs as a dict of Python floats / ints (the fp32 values, exactly)."""
    return {name: getattr(k, name) for name, _ in k._fields_}


def xp(k, x, eps, xt=None, ew=None, ec=None):
    """The step's clean estimate before its clamp, after the ROI edit when one is on (ew: (H, W), ec: (3, H, W))."""
    k = coefs(k) if not isinstance(k, dict) else k
    x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    x0 = k["sqrt_recip_ac_t"] * x - k["sqrt_recipm1_ac_t"] * eps
    if k["mode"] != 0:
        x0 = (x0 - k["gamma_t"] * np.asarray(xt, np.float64)) / (1.0 - k["gamma_t"])
    if ew is not None:
        x0 = np.asarray(ew, np.float64) * x0 + np.asarray(ec, np.float64)
    return x0


def block_mean(r, N, halo=(0, 0)):
    """M: (..., H, W) -> (..., h, w), the mean over the centre pixels of every N x N block; a partial edge block divides
    by its own pixel count; the block grid starts at the halo and halo pixels are not read."""
    r = np.asarray(r, np.float64)
    hy, hx = halo
    Hc, Wc = r.shape[-2] - 2 * hy, r.shape[-1] - 2 * hx
    h, w = -(-Hc // N), -(-Wc // N)
    out = np.empty(r.shape[:-2] + (h, w), np.float64)
    for Y in range(h):
        for X in range(w):
            blk = r[..., hy + Y * N:hy + min((Y + 1) * N, Hc), hx + X * N:hx + min((X + 1) * N, Wc)]
            out[..., Y, X] = blk.sum(axis=(-2, -1)) / (blk.shape[-2] * blk.shape[-1])
    return out


def _axis(size_buf, halo, size_c, N, n, wrap):
    """Per buffer coordinate: (i0, i1, weight of i1)."""
    v = np.arange(size_buf) - halo
    if wrap:
        v = np.mod(v, size_c)
    f = (v + 0.5) / N - 0.5
    if wrap:
        fl = np.floor(f)
        i0 = np.mod(fl.astype(np.int64), n)
        return i0, np.mod(i0 + 1, n), f - fl
    f = np.clip(f, 0.0, n - 1.0)
    i0 = np.floor(f).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), f - i0


def upsample(D, N, Hc, Wc, halo=(0, 0), wrap=(False, False)):
    """U: (..., h, w) -> (..., H, W), bilinear interpolation between block centres."""
    D = np.asarray(D, np.float64)
    hy, hx = halo
    h, w = D.shape[-2], D.shape[-1]
    assert (h, w) == (-(-Hc // N), -(-Wc // N))
    y0, y1, ly = _axis(Hc + 2 * hy, hy, Hc, N, h, bool(wrap[0]) or hy != 0)
    x0, x1, lx = _axis(Wc + 2 * hx, hx, Wc, N, w, bool(wrap[1]) or hx != 0)
    ly, lx = ly[:, None], lx[None, :]
    top = (1.0 - lx) * D[..., y0[:, None], x0[None, :]] + lx * D[..., y0[:, None], x1[None, :]]
    bot = (1.0 - lx) * D[..., y1[:, None], x0[None, :]] + lx * D[..., y1[:, None], x1[None, :]]
    return (1.0 - ly) * top + ly * bot


def delta(k, L, x, eps, xt=None, ew=None, ec=None, N=8, halo=(0, 0)):
    """D[b, ch, Y, X]: block mean of L[ch] - xp[b, ch]."""
    return block_mean(np.asarray(L, np.float64)[None] - xp(k, x, eps, xt, ew, ec), N, halo)


def step(k, x, eps, xt, z, w, c, keep=None):
    """The reverse step with the edit  x_recon <- w * x_recon + c  (w, c broadcastable arrays; c = c_eff) in float64:
    predict_start_from_noise + p_mean_variance + q_posterior as the project's step evaluates them, then the keep blend
    (keep = (m, k0, ka, kb)) on the output."""
    k = coefs(k) if not isinstance(k, dict) else k
    x, eps, z = (np.asarray(a, np.float64) for a in (x, eps, z))
    clamp = (lambda a: np.clip(a, -1.0, 1.0)) if k["clip"] else (lambda a: a)
    x0 = k["sqrt_recip_ac_t"] * x - k["sqrt_recipm1_ac_t"] * eps
    xb = None if k["mode"] == 0 else np.asarray(xt, np.float64)
    if k["mode"] == 0:
        mean = k["coef1_t"] * clamp(w * x0 + c) + k["coef2_t"] * x
    else:
        est = w * ((x0 - k["gamma_t"] * xb) / (1.0 - k["gamma_t"])) + c
        if k["mode"] == 1:
            mix = clamp(k["gamma_tm1"] * xb + (1.0 - k["gamma_tm1"]) * est)
            mean = k["sqrt_ac_tm1"] * mix + k["sqrt_1m_ac_tm1_mvar"] * (x - k["sqrt_ac_t"] * clamp(x0)) / k["sqrt_1m_ac_t"]
        else:
            mean = clamp(est)
    out = mean + k["sigma"] * z
    if keep is not None:
        m, k0, ka, kb = keep
        m, k0 = np.asarray(m, np.float64), np.asarray(k0, np.float64)
        target = k["gamma_tm1"] * xb + (1.0 - k["gamma_tm1"]) * k0 if k["mode"] == 1 else k0
        out = m * (ka * target + kb * z) + (1.0 - m) * out
    return out


def layout_step(k, x, eps, xt, z, D, g, N, ew=None, ec=None, keep=None, halo=(0, 0), wrap=(False, False)):
    """The conditioned step: c_eff = ec + g * U(D)."""
    H, W = x.shape[-2], x.shape[-1]
    U = upsample(D, N, H - 2 * halo[0], W - 2 * halo[1], halo, wrap)
    w = 1.0 if ew is None else np.asarray(ew, np.float64)
    c = g * U + (0.0 if ec is None else np.asarray(ec, np.float64))
    return step(k, x, eps, xt, z, w, c, keep)
