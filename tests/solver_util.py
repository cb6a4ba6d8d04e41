"""Float64 restatement of few-step sampling -- the strided reverse step and the second-order multistep step -- written from
the formulas of include/sinddm_hip.h ("few-step sampling") and DESIGN.md 3, not from the kernel.  Shared by
tests/test_solver_host.py and tests/test_gpu_solver.py.

Conventions (those of tests/resample_util.py): sa / sb are sqrt(ac) / sqrt(1 - ac) of the schedule's alphas_cumprod, gamma
the sampling gamma of the scale clamped to [0, 0.55] (zeros in mode 0); the marginal at level l is  sa[l] * M_l + sb[l] * eps,
M_l = gamma[l] * x_tilde + (1 - gamma[l]) * x0;  kappa[l] = sa[l] * (1 - gamma[l]) / sb[l].  A step from level t lands on
level u < t; u = -1 is the clean image.  The step t -> t - 1 with eta = 1 is the oracle's `reverse_step` (through
resample_util.step_jump_ref, which adds the known-region replacement); every other landing is restated here.
"""
import numpy as np
import torch

from resample_util import levels, step_jump_ref


def kappa(d, s):
    sa, sb, g = levels(d, s)
    return sa * (1.0 - g) / sb


def solver_q(d, s, taus, lands):
    """q_i = rho_i * (1 - gamma[tau_i]) * sa[tau_i] / sb[tau_i], rho_i = ln(kappa[u_i] / kappa[tau_i]) /
    (2 ln(kappa[tau_i] / kappa[tau_{i-1}])); 0 on the first step and on a step that lands clean."""
    sa, sb, g = levels(d, s)
    kap = kappa(d, s)
    out = []
    for i, (t, u) in enumerate(zip(taus, lands)):
        if i == 0 or u < 0:
            out.append(0.0)
            continue
        rho = np.log(kap[u] / kap[t]) / (2.0 * np.log(kap[t] / kap[taus[i - 1]]))
        out.append(float(rho * (1.0 - g[t]) * sa[t] / sb[t]))
    return out


def clean_estimate(d, s, t, x, eps, x_tilde):
    """xp of a step: the clean image the pair (x, eps) implies at level t, before any edit or clamp (float64 in and out)."""
    sa, sb, g = levels(d, s)
    x0 = (x - float(sb[t]) * eps) / float(sa[t])               # (1 / sa, sb / sa: the float64 forms of the two fp32 tables)
    if int(s) == 0 or not d.reblurring:
        return x0
    return (x0 - float(g[t]) * x_tilde) / (1.0 - float(g[t]))


def step_to_ref(d, s, t, u, x, eps, x_tilde, z, edit=None, keep=None, clip=True, eta=1.0, q=0.0, hist=None, dtype=torch.float64):
    """The reverse step of scale s from level t to level u (u = -1: clean), multistep factor q with `hist` the previous
    step's clean estimate (read only when q != 0).  Tensors of any float dtype / device; (B,3,H,W) states, edit = (w (H,W),
    c (3,H,W)), keep = (m (H,W), k0 (3,H,W)).  Returns (out, xp): CPU tensors of `dtype`, xp this step's own clean estimate.
    `dtype` = torch.float32 evaluates the same expressions in fp32 (strided landings only): the rounding an fp32
    implementation cannot avoid."""
    f = lambda v: None if v is None else v.detach().cpu().to(dtype)
    x, eps, x_tilde, z, hist = f(x), f(eps), f(x_tilde), f(z), f(hist)
    t, u, s = int(t), int(u), int(s)
    assert -1 <= u < t
    xp = clean_estimate(d, s, t, x, eps, x_tilde)
    e2 = eps - float(q) * (xp - hist) if q != 0.0 else eps
    if u == t - 1 and float(eta) == 1.0:
        assert dtype == torch.float64
        return step_jump_ref(d, s, t, None, x, e2, x_tilde, z, None, edit=edit, keep=keep, clip=clip), xp
    sa, sb, g = levels(d, s)
    mode0 = s == 0 or not d.reblurring
    x0 = (x - float(sb[t]) * e2) / float(sa[t])
    est = x0 if mode0 else (x0 - float(g[t]) * x_tilde) / (1.0 - float(g[t]))
    if edit is not None:
        est = f(edit[0])[None, None] * est + f(edit[1])[None]
    cl = (lambda v: v.clamp(-1.0, 1.0)) if clip else (lambda v: v)
    if u < 0:
        out = cl(est)
    elif mode0:
        ac_t, ac_u = sa[t] ** 2, sa[u] ** 2
        sigma = float(eta) * np.sqrt((1.0 - ac_u) / (1.0 - ac_t)) * np.sqrt(1.0 - ac_t / ac_u)
        coef2 = np.sqrt(sb[u] ** 2 - sigma ** 2) / sb[t]
        x0c = cl(est)
        out = float(sa[u]) * x0c + float(coef2) * (x - float(sa[t]) * x0c) + float(sigma) * z
    else:
        mix = cl(float(g[u]) * x_tilde + (1.0 - float(g[u])) * est)
        var = float(d.omega) * (1.0 - sa[u] ** 2)
        out = (float(sa[u]) * mix + float(np.sqrt(1.0 - sa[u] ** 2 - var)) * (x - float(sa[t]) * cl(x0)) / float(sb[t])
               + float(np.sqrt(max(var, 1e-20))) * z)
    if keep is not None:
        m, k0 = f(keep[0])[None, None], f(keep[1])[None]
        if u < 0:
            kept = k0.expand_as(x)
        else:
            target = k0 if mode0 else float(g[u]) * x_tilde + (1.0 - float(g[u])) * k0
            kept = float(sa[u]) * target + float(sb[u]) * z
        out = m * kept + (1.0 - m) * out
    return out, xp


def run_ref(d, s, taus, lands, x, eps_fn, order=1, x_tilde=None, clip=False, eta=1.0, z_fn=None, round32=False):
    """A whole run in float64: eps_fn(x, t) is the denoiser, z_fn(i) the step's draw (None: zeros).  `round32` rounds the
    state, eps and the history to fp32 after every step: the floor an fp32 implementation of the same loop cannot beat."""
    q = solver_q(d, s, taus, lands) if order == 2 else [0.0] * len(taus)
    r = (lambda v: v.float().double()) if round32 else (lambda v: v)
    x, hist = r(x.double()), None
    for i, (t, u) in enumerate(zip(taus, lands)):
        z = z_fn(i) if z_fn is not None else torch.zeros_like(x)
        x, hist = step_to_ref(d, s, t, u, x, r(eps_fn(x, t)), x_tilde, z, clip=clip, eta=eta, q=float(np.float32(q[i])) if round32 else q[i],
                              hist=hist)
        x, hist = r(x), r(hist)
    return x


class Gaussian:
    """Data N(mu, sd^2) per element under SinDDM's blurred process with a constant x-tilde: the analytic denoiser and the
    exact probability-flow solution (a Gaussian marginal is transported by the affine map that keeps the standardised
    coordinate)."""

    def __init__(self, d, s, mu=0.3, sd=0.5, xt=-0.2):
        self.sa, self.sb, self.g = levels(d, s)
        self.mu, self.sd, self.xt = mu, sd, xt

    def mean_var(self, l):
        if l < 0:
            return self.mu, self.sd ** 2
        sa, sb, g = self.sa[l], self.sb[l], self.g[l]
        return sa * (g * self.xt + (1.0 - g) * self.mu), (sa * (1.0 - g) * self.sd) ** 2 + sb ** 2

    def sample(self, l, x0, eps):
        sa, sb, g = self.sa[l], self.sb[l], self.g[l]
        return sa * (g * self.xt + (1.0 - g) * x0) + sb * eps

    def eps(self, x, l):
        """(x - sa * M(E[x0 | x])) / sb at level l; any dtype / device in, the same out."""
        sa, sb, g = float(self.sa[l]), float(self.sb[l]), float(self.g[l])
        m, v = self.mean_var(l)
        x0 = self.mu + sa * (1.0 - g) * self.sd ** 2 * (x - float(m)) / float(v)
        return (x - sa * (g * self.xt + (1.0 - g) * x0)) / sb

    def exact(self, x, l_from, l_to):
        m0, v0 = self.mean_var(l_from)
        m1, v1 = self.mean_var(l_to)
        return float(m1) + float(np.sqrt(v1 / v0)) * (x - float(m0))


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())
