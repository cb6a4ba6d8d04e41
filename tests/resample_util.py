"""Float64 restatement of a reverse step followed by a resampling jump, written from the formulas of include/sinddm_hip.h
("resampling jumps") and DESIGN.md 3, not from the kernel.  Shared by tests/test_resample_host.py and
tests/test_gpu_resample.py.

Conventions: a reverse step at index t > 0 takes a state at noise level t and writes one at level l = t - 1.  sa / sb are
sqrt(ac) / sqrt(1 - ac) of the schedule's alphas_cumprod, gamma the sampling gamma of the scale clamped to [0, 0.55] (zeros in
mode 0).  The marginal at level l is  sa[l] * M_l + sb[l] * eps,  M_l = gamma[l] * x_tilde + (1 - gamma[l]) * x0.  The jump
from l to l2 >= l is  out = r * y + s * z2 + d * (x_tilde - x0h)  with r = sa[l2] / sa[l], s = sqrt(1 - r^2),
d = sa[l2] * (gamma[l2] - gamma[l]).

The step itself is the oracle's `reverse_step` (the reference's p_sample after the network call) run in float64 on the
diffusion's own host tables; the known-region replacement and the jump are restated here.
"""
import numpy as np
import torch

from oracle import sinddm_oracle as O

_SCHED_KEYS = ("alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
               "sqrt_recipm1_alphas_cumprod", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2",
               "gammas")


def sched64(d):
    """The schedule the oracle's reverse_step reads, from the diffusion's registered (fp32) tables, as float64 tensors."""
    return {k: getattr(d, k).detach().cpu().double() for k in _SCHED_KEYS}


def levels(d, s):
    """(sa, sb, gamma): float64 numpy arrays over the noise levels of scale s."""
    ac = d.alphas_cumprod.detach().cpu().double().numpy()
    if int(s) == 0 or not d.reblurring:
        g = np.zeros_like(ac)
    else:
        g = np.clip(d.gammas[int(s) - 1].detach().cpu().double().numpy().reshape(-1), 0.0, float(np.float32(0.55)))
    return np.sqrt(ac), np.sqrt(1.0 - ac), g


def jump_coefs(d, s, l, l2):
    sa, _, g = levels(d, s)
    r = sa[l2] / sa[l]
    return float(r), float(np.sqrt(1.0 - r * r)), float(sa[l2] * (g[l2] - g[l]))


def level_mean(d, s, l, x_tilde, x0):
    """M_l of the marginal (float64 tensors in, float64 tensor out); x_tilde may be None in mode 0."""
    _, _, g = levels(d, s)
    return x0 if g[l] == 0.0 and x_tilde is None else float(g[l]) * x_tilde + (1.0 - float(g[l])) * x0


def step_jump_ref(d, s, t, l2, x, eps, x_tilde, z, z2, edit=None, keep=None, clip=True):
    """Reverse step t of scale s followed by the jump from level t - 1 to level l2 (None: the step alone).  Tensors of any
    float dtype / device; (B,3,H,W) states, edit = (w (H,W), c (3,H,W)), keep = (m (H,W), k0 (3,H,W)).  Returns a float64
    CPU tensor."""
    f = lambda v: None if v is None else v.detach().cpu().double()
    x, eps, x_tilde, z, z2 = f(x), f(eps), f(x_tilde), f(z), f(z2)
    t, s = int(t), int(s)
    assert t > 0 or l2 is None, "no jump after the step t = 0"
    mode0 = s == 0 or not d.reblurring
    sch = sched64(d)
    edit_fn = None
    if edit is not None:
        w, c = f(edit[0]), f(edit[1])
        edit_fn = lambda v: w[None, None] * v + c[None]
    y = O.reverse_step(sch, x, eps, t, s, z, x_tilde, reblurring=d.reblurring, omega=float(d.omega), clip_denoised=clip,
                       x_recon_edit=edit_fn)
    sa, sb, g = levels(d, s)
    m = k0 = None
    if keep is not None:
        m, k0 = f(keep[0])[None, None], f(keep[1])[None]
        if t > 0:
            target = k0 if mode0 else float(g[t - 1]) * x_tilde + (1.0 - float(g[t - 1])) * k0
            kept = float(sa[t - 1]) * target + float(sb[t - 1]) * z
        else:
            kept = k0.expand_as(x)
        y = m * kept + (1.0 - m) * y
    if l2 is None:
        return y
    l = t - 1
    r, sj, dj = jump_coefs(d, s, l, int(l2))
    out = r * y + sj * z2
    if not mode0:
        x0 = sch["sqrt_recip_alphas_cumprod"][t] * x - sch["sqrt_recipm1_alphas_cumprod"][t] * eps
        xp = (x0 - float(g[t]) * x_tilde) / (1.0 - float(g[t]))
        if edit_fn is not None:
            xp = edit_fn(xp)
        if clip:
            xp = xp.clamp(-1.0, 1.0)
        x0h = xp if keep is None else m * k0 + (1.0 - m) * xp
        out = out + dj * (x_tilde - x0h)
    return out


def whitened(out, d, s, l2, x_tilde, x0):
    """(out - sa[l2] * M_l2) / sb[l2]: N(0,1) per element when `out` has the level-l2 marginal of clean image x0."""
    sa, sb, _ = levels(d, s)
    f = lambda v: None if v is None else v.detach().cpu().double()
    return (f(out) - float(sa[l2]) * level_mean(d, s, l2, f(x_tilde), f(x0))) / float(sb[l2])


def moment_limits(n):
    """(|mean| limit, |variance - 1| limit) of n independent N(0,1) values at five standard errors."""
    return 5.0 / np.sqrt(n), 5.0 * np.sqrt(2.0 / n)


def closed_form_count(t_seq, R, J):
    """len(t_seq) + (R - 1) * J * |anchors|: anchors = levels t - 1 >= 0 reached by the run that are multiples of J with
    l + J <= t_seq[0]."""
    t_seq = list(t_seq)
    L = t_seq[0]
    anchors = [t - 1 for t in t_seq if t - 1 >= 0 and (t - 1) % J == 0 and t - 1 + J <= L]
    return len(t_seq) + (R - 1) * J * len(anchors)
