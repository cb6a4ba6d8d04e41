"""Few-step sampling, host side (no GPU): the strided schedules (functions.stride_schedule), the strided step scalars
(`step_coefs_to`), the marginal a strided step must land on and the order of accuracy of the multistep step -- in float64
through tests/solver_util.py -- and the new argument checks of the chain call (chain_run.h), through the library on fake
pointers and in a stand-alone program under the host sanitizers.

Shapes: the float64 tests run on a few thousand elements (moments: 3 x 64 x 64 = 12 288, enough for five standard errors to
be tight; order: 4096, the issue's count).  C2 is the schedule whose gamma saturates inside the runs used here.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from resample_util import levels, moment_limits
from sinddm_amd import _lib
from sinddm_amd.configs import build_diffusion
from sinddm_amd.functions import stride_schedule
from solver_util import Gaussian, kappa, rms, run_ref, solver_q, step_to_ref
from test_batch_maps_host import REPO, _host_cxx
from test_chain_run_host import BADARG, JUMP, LAY, P, WORKSPACE


@pytest.fixture(scope="module")
def c2():
    return build_diffusion("C2", dim=20)[1]


# ---- 1: schedules --------------------------------------------------------------------------------------------------------
def test_stride_schedule(c2):
    kap = kappa(c2, 3)
    run = list(range(311, -1, -1))
    for spacing in ("t", "logsnr"):
        for n in (len(run), len(run) + 5):                                     # n >= len: the identity
            assert stride_schedule(run, n, spacing, kap) == (run, [t - 1 for t in run])
        for seq, n in ((run, 10), (run, 40), (run, 2), (list(range(200, 49, -1)), 7), (run, 300)):
            taus, lands = stride_schedule(seq, n, spacing, kap)
            assert taus[0] == seq[0] and taus[-1] == seq[-1] and lands == taus[1:] + [seq[-1] - 1]
            assert 2 <= len(taus) <= n and all(a > b for a, b in zip(taus, taus[1:]))      # strictly descending
            assert set(taus) <= set(seq)
        assert stride_schedule(run, 1, spacing, kap) == ([311], [-1])         # n = 1: one step, level 311 to the clean image
        assert stride_schedule([7], 1, spacing, kap) == ([7], [6]) and stride_schedule([], 3, spacing, kap) == ([], [])
    assert stride_schedule(run, 5, "t") == ([311, 233, 156, 78, 0], [233, 156, 78, 0, -1])
    # 'logsnr' drops duplicates: log kappa changes fastest at the low levels, so asking for nearly every level of the run
    # names some high level twice
    taus, _ = stride_schedule(run, 300, "logsnr", kap)
    assert len(taus) < 300 and len(set(taus)) == len(taus)
    # ... and is equally spaced in log kappa where 't' is not
    lam = lambda ts: np.diff(np.log(kap[ts]))
    ls, lt = lam(stride_schedule(run, 10, "logsnr", kap)[0]), lam(stride_schedule(run, 10, "t")[0])
    assert ls.max() / ls.min() < 1.3 < lt.max() / lt.min()
    bad = kap.copy()
    bad[100] = bad[101]                                                         # does not rise between levels 101 and 100
    with pytest.raises(ValueError):
        stride_schedule(run, 10, "logsnr", bad)
    for kw in (dict(n=0), dict(spacing="x"), dict(spacing="logsnr")):          # (no kappa)
        with pytest.raises(ValueError):
            stride_schedule(run, **{"n": 10, **kw})
    with pytest.raises(ValueError):
        stride_schedule([5, 3, 2], 2)
    assert bool(np.all(np.diff(kap) < 0)) and bool(np.all(np.diff(kappa(c2, 0)) < 0))      # the real tables do rise


# ---- 2: strided step scalars ---------------------------------------------------------------------------------------------
FIELDS = [f for f, _ in _lib.StepCoefs._fields_]


def test_step_coefs_to_reduces_to_step_coefs(c2):
    d = c2
    for omega in (0.0, 0.3):
        d.omega = omega
        for s in (0, 1):
            for t in range(d.num_timesteps):
                for clip in (True, False):
                    a, b = d.step_coefs_to(t, t - 1, s, clip), d.step_coefs(t, s, clip)
                    assert all(getattr(a, f) == getattr(b, f) for f in FIELDS), (s, t)
    d.omega = 0.0
    # the clean landing
    k = d.step_coefs_to(700, -1, 0)
    assert (k.mode, k.coef1_t, k.coef2_t, k.sigma) == (0, 1.0, 0.0, 0.0)
    assert k.sqrt_recip_ac_t == d.step_coefs(700, 0).sqrt_recip_ac_t
    k, k1 = d.step_coefs_to(200, -1, 1), d.step_coefs(200, 1)
    assert k.mode == 2 and k.sigma == 0.0
    assert (k.gamma_t, k.sqrt_recip_ac_t, k.sqrt_recipm1_ac_t) == (k1.gamma_t, k1.sqrt_recip_ac_t, k1.sqrt_recipm1_ac_t)
    # mode 0 strided: the DDIM form in float64, eta scales sigma; eta = 1 at u = t - 1 is the posterior to table rounding
    sa, sb, _ = levels(d, 0)
    for eta in (0.0, 0.5, 1.0):
        k = d.step_coefs_to(700, 400, 0, eta=eta)
        sigma = eta * np.sqrt((1 - sa[400] ** 2) / (1 - sa[700] ** 2)) * np.sqrt(1 - sa[700] ** 2 / sa[400] ** 2)
        coef2 = np.sqrt(sb[400] ** 2 - sigma ** 2) / sb[700]
        assert k.mode == 0 and abs(k.sigma - sigma) < 1e-7 and abs(k.coef2_t - coef2) < 1e-7
        assert abs(k.coef1_t - (sa[400] - coef2 * sa[700])) < 1e-7
    k0, kp = d.step_coefs_to(700, 699, 0, eta=1.0 + 1e-12), d.step_coefs(700, 0)            # (past the shortcut)
    assert abs(k0.coef1_t - kp.coef1_t) < 1e-6 and abs(k0.coef2_t - kp.coef2_t) < 1e-6 and abs(k0.sigma - kp.sigma) < 1e-6
    # mode 1 strided: the tm1 fields take level u
    d.omega = 0.3
    k, ku = d.step_coefs_to(200, 50, 1), d.step_coefs(51, 1)
    assert k.mode == 1 and all(getattr(k, f) == getattr(ku, f) for f in ("gamma_tm1", "sqrt_ac_tm1", "sqrt_1m_ac_tm1_mvar", "sigma"))
    assert all(getattr(k, f) == getattr(d.step_coefs(200, 1), f) for f in ("gamma_t", "sqrt_ac_t", "sqrt_1m_ac_t", "sqrt_recip_ac_t"))
    assert k.gamma_tm1 != k.gamma_t
    d.omega = 0.0
    for bad in ((5, 5), (5, 7), (5, -2), (1000, 3)):
        with pytest.raises(ValueError):
            d.step_coefs_to(*bad, 1)
    # the multistep factors are the formula's
    taus, lands = stride_schedule(list(range(311, -1, -1)), 6, "logsnr", kappa(d, 3))
    q = d._solver_q(3, taus, lands)
    assert q[0] == 0.0 and q[-1] == 0.0 and all(v > 0 for v in q[1:-1])
    assert np.allclose(q, solver_q(d, 3, taus, lands), rtol=1e-12, atol=0)


# ---- 3: marginal consistency ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,t,u", [(0, 700, 400), (1, 200, 50)], ids=["scale0", "scale1"])
def test_strided_step_lands_on_the_marginal(c2, s, t, u):
    d = c2
    shape = (1, 3, 64, 64)
    g = torch.Generator().manual_seed(5 + s)
    x0, eps, z = (torch.randn(shape, generator=g, dtype=torch.float64) * a for a in (0.5, 1.0, 1.0))
    xt = torch.randn(shape, generator=g, dtype=torch.float64) * 0.4 if s > 0 else None
    sa, sb, gm = levels(d, s)
    M = lambda l: x0 if s == 0 else float(gm[l]) * xt + (1 - float(gm[l])) * x0
    x = float(sa[t]) * M(t) + float(sb[t]) * eps
    d.omega = 0.0
    # eps handed in as the prediction, sigma = 0 (no draw: at a scale > 0 the reference floors sigma at 1e-10, not at 0)
    zero = torch.zeros_like(z)
    out, xp = step_to_ref(d, s, t, u, x, eps, xt, zero, clip=False, eta=0.0)
    err = float((out - (float(sa[u]) * M(u) + float(sb[u]) * eps)).abs().max())
    print(f"s={s} {t} -> {u}: deterministic strided step vs the level-{u} marginal max-abs {err:.3e}")
    assert err <= 1e-12 and float((xp - x0).abs().max()) <= 1e-12
    # ... and the clean landing returns the clean image
    out, _ = step_to_ref(d, s, t, -1, x, eps, xt, zero, clip=False, eta=0.0)
    assert float((out - x0).abs().max()) <= 1e-12
    # with noise: the whitened output is N(0, 1)
    d.omega = 0.3
    out, _ = step_to_ref(d, s, t, u, x, eps, xt, z, clip=False, eta=1.0)
    d.omega = 0.0
    wz = (out - float(sa[u]) * M(u)) / float(sb[u])
    mean, var = float(wz.mean()), float(wz.var(unbiased=False))
    lim_m, lim_v = moment_limits(wz.numel())
    print(f"    noisy: whitened mean {mean:+.5f} (limit {lim_m:.5f}) variance {var:.5f} (1 +- {lim_v:.5f})")
    assert abs(mean) <= lim_m and abs(var - 1.0) <= lim_v
    assert float((out - (float(sa[u]) * M(u) + float(sb[u]) * eps)).abs().max()) > 1e-2      # (the draw is in it)


# ---- 4: order on the analytic Gaussian ------------------------------------------------------------------------------------
def gaussian_problem(d, n=4096, shape=(1, 1, 64, 64)):
    """Data N(0.3, 0.5^2), x-tilde = -0.2, C2 scale 3 from level 311 to the clean image: (G, x at level 311, x-tilde, exact)."""
    G = Gaussian(d, 3)
    g = torch.Generator().manual_seed(1)
    x0 = 0.3 + 0.5 * torch.randn(n, generator=g, dtype=torch.float64)
    e = torch.randn(n, generator=g, dtype=torch.float64)
    x = G.sample(311, x0, e).view(shape).contiguous()
    return G, x, torch.full_like(x, -0.2), G.exact(x, 311, -1)


def order_conditions(e1, e2, e2_log10, slack=0.0):
    """The issue's conditions on e1(N), e2(N) (dicts over N, t-spaced) and e2(10) log-SNR-spaced; `slack`: the fp32 floor
    an implementation may add to its e2 values (0 in float64)."""
    print(f"e1: { {n: f'{v:.3e}' for n, v in e1.items()} }  e2: { {n: f'{v:.3e}' for n, v in e2.items()} }  "
          f"e2(10, logsnr): {e2_log10:.3e}  slack {slack:.1e}")
    print(f"e1(40)/e2(40) = {e1[40] / e2[40]:.2f} (> 3)   e2(20)/e2(40) = {e2[20] / e2[40]:.2f} (> 3)   "
          f"e1(20)/e1(40) = {e1[20] / e1[40]:.2f} (< 2.5)")
    assert e2[40] - slack < e1[40] / 3
    assert e2[20] + slack > 3 * (e2[40] - slack)
    assert e1[20] < 2.5 * e1[40]
    assert e2_log10 - slack < e1[40]


def test_order_on_the_analytic_gaussian(c2):
    d = c2
    assert d.omega == 0
    G, x, xt, exact = gaussian_problem(d)
    run, kap = list(range(311, -1, -1)), kappa(d, 3)
    e = {}
    for order in (1, 2):
        e[order] = {n: rms(run_ref(d, 3, *stride_schedule(run, n, "t"), x, G.eps, order, x_tilde=xt), exact) for n in (20, 40)}
    e2_log = rms(run_ref(d, 3, *stride_schedule(run, 10, "logsnr", kap), x, G.eps, 2, x_tilde=xt), exact)
    order_conditions(e[1], e[2], e2_log)
    # every level, first order: the reference's own run converges to the same solution
    assert rms(run_ref(d, 3, run, [t - 1 for t in run], x, G.eps, 1, x_tilde=xt), exact) < e[1][40] / 5


# ---- 5: the chain call's new checks -----------------------------------------------------------------------------------------
def _solver_call(q=(0.0, 0.5), hist=P, modes=(1, 0), jumps=None, lay=None, so_null=False, q_null=False):
    lib = _lib.load()
    coefs = (_lib.StepCoefs * 2)()
    coefs[0].mode, coefs[1].mode = modes
    tl = (C.c_int * 2)(5, 2)
    flag = C.c_int(7)
    qarr = (C.c_float * 2)(*q)
    so = _lib.SolverOpts(None if q_null else C.cast(qarr, C.POINTER(C.c_float)), hist)
    jarr = (_lib.JumpCoefs * 2)(*[_lib.JumpCoefs(*j) for j in jumps]) if jumps else None
    ro = _lib.ResampleOpts(jarr, None) if jumps else None
    garr = (C.c_float * 2)(*lay[2]) if lay else None
    lo = _lib.LayoutOpts(lay[0], lay[1], garr, lay[3]) if lay else None
    ref = lambda o: C.byref(o) if o is not None else None
    rc = lib.sinddm_sample_chain_solver(P, P, P, P, P, P, coefs, tl, 2, 0.0, 1, 0, 160, 4, 8, 8, P, 0, None, None, C.byref(flag),
                                        None, 0, 0, None, None, ref(ro), ref(lo), None, None if so_null else C.byref(so))
    assert flag.value == 7                                                     # nothing was run
    return rc


def test_solver_checks_through_the_library():
    # a valid block passes every check: the empty workspace is reported, last
    assert _solver_call() == WORKSPACE
    assert _solver_call(so_null=True) == WORKSPACE and _solver_call(q_null=True, hist=None) == WORKSPACE
    assert _solver_call(q=(0.0, 0.0), modes=(1, 2)) == WORKSPACE               # q = 0 on the mode-2 step is the plain step
    assert _solver_call(q_null=True, hist=P + 4) == WORKSPACE                  # without q the block is not read
    bad = [dict(hist=None), dict(hist=P + 4), dict(hist=P + 8), dict(q=(0.0, -0.5)), dict(q=(float("inf"), 0.0)),
           dict(q=(0.0, float("nan"))), dict(q=(0.0, 0.5), modes=(1, 2)), dict(jumps=JUMP, modes=(0, 0)),
           dict(lay=LAY), dict(lay=(P, 4, (0.0, 0.25), P))]
    for kw in bad:
        assert _solver_call(**kw) == BADARG, kw
    # jumps none of which is on, and a layout that never pulls, are the call without them
    assert _solver_call(jumps=[(0, 9.0, -1.0, 0.0)] * 2) == WORKSPACE
    assert _solver_call(lay=(P, 4, (0.0, 0.0), P)) == WORKSPACE
    # the single-step entry
    lib = _lib.load()
    k = _lib.StepCoefs()
    call = lambda q, hist=P, mode=1: lib.sinddm_reverse_step_ms(P, P, P, P, P, C.byref(_coefs(mode)), q, hist, None, None, None, None,
                                                                 1.0, 0.0, 2, 3, 35, None)
    _coefs = lambda mode: _lib.StepCoefs(mode=mode)
    assert call(-1.0) == BADARG and call(float("nan")) == BADARG and call(float("inf")) == BADARG
    assert call(0.5, hist=None) == BADARG and call(0.5, mode=2) == BADARG
    assert lib.sinddm_reverse_step_ms(P, P, None, P, P, C.byref(k), 0.0, P, P, None, None, None, 1.0, 0.0, 2, 3, 35, None) == BADARG


SAN_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include "chain_run.h"
using namespace sinddm;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
alignas(16) static float dev[64];                               // stands for device memory: only its addresses are used
static sinddm_step_coefs coefs[3];                              // modes 1, 1, 2: the end of a scale's walk
static int tl[3] = {9, 4, 0};
static ChainRun plain() {
    coefs[0].mode = coefs[1].mode = 1; coefs[2].mode = 2;
    return chain_run_fill(dev, dev, dev, dev, dev, dev, coefs, tl, 3, 0.0f, 1, 0, 160, 4, 8, 12, dev, 0, nullptr, nullptr, nullptr);
}
template <class F> static int with(F&& f, ChainChecked* c = nullptr) {
    ChainRun r = plain();
    f(r);
    ChainChecked local;
    return chain_check(r, c ? c : &local);
}
int main() {
    static const float q[3] = {0.0f, 0.75f, 0.0f}, q_neg[3] = {0.0f, -0.75f, 0.0f}, q_last[3] = {0.0f, 0.5f, 0.5f};
    static const float q_inf[3] = {std::numeric_limits<float>::infinity(), 0.0f, 0.0f}, q_nan[3] = {0.0f, std::nanf(""), 0.0f};
    static const sinddm_jump_coefs jmp[3] = {{1, 0.5f, 0.5f, 0.25f}, {0, 0, 0, 0}, {0, 0, 0, 0}}, joff[3] = {{0, 9, -1, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    static const float g[3] = {1.0f, 0.0f, 0.5f}, g_off[3] = {0, 0, 0};
    float* hist = dev + 4;                                      // 16-byte aligned
    ChainChecked c;
    CHECK(with([](ChainRun&) {}, &c) == 0 && !c.ms_q);                                              // no block
    CHECK(with([&](ChainRun& r) { r.solver_hist = dev + 1; }, &c) == 0 && !c.ms_q);                 // hist alone is not read
    CHECK(with([&](ChainRun& r) { r.solver_q = q; r.solver_hist = hist; }, &c) == 0 && c.ms_q == q);
    CHECK(with([&](ChainRun& r) { r.solver_q = q; }) == SINDDM_E_BADARG);                           // q without hist
    CHECK(with([&](ChainRun& r) { r.solver_q = q; r.solver_hist = dev + 1; }) == SINDDM_E_BADARG);  // misaligned
    CHECK(with([&](ChainRun& r) { r.solver_q = q; r.solver_hist = dev + 2; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.solver_q = q_neg; r.solver_hist = hist; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.solver_q = q_inf; r.solver_hist = hist; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.solver_q = q_nan; r.solver_hist = hist; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.solver_q = q_last; r.solver_hist = hist; }) == SINDDM_E_BADARG);             // q != 0 on the mode-2 step
    CHECK(with([&](ChainRun& r) { r.solver_q = q_last; r.solver_hist = hist; r.n_steps = 2; }, &c) == 0 && c.ms_q == q_last);
    CHECK(with([&](ChainRun& r) { r.solver_q = q; r.solver_hist = hist; r.jumps = jmp; }) == SINDDM_E_BADARG);   // a jump is on
    CHECK(with([&](ChainRun& r) { r.solver_q = q; r.solver_hist = hist; r.jumps = joff; }, &c) == 0 && c.ms_q == q && !c.jumps);
    CHECK(with([&](ChainRun& r) { r.solver_q = q; r.solver_hist = hist; r.layout = dev; r.layout_g = g; r.layout_down = 4; r.layout_delta = dev; }) ==
          SINDDM_E_BADARG);                                                                                      // a step pulls
    CHECK(with([&](ChainRun& r) { r.solver_q = q; r.solver_hist = hist; r.layout = dev; r.layout_g = g_off; }, &c) == 0 && c.ms_q == q);
    CHECK(with([&](ChainRun& r) { r.solver_q = q; r.x = nullptr; }) == SINDDM_E_BADARG);
    // the block through chain_run_set, NULL-tolerant, beside every other option
    sinddm_solver_opts so{q, hist};
    sinddm_chain_opts o{dev, dev, dev};
    sinddm_batch_opts bo{1, 1, 1, 0, nullptr};
    ChainRun r = plain();
    chain_run_set(r, &o); chain_run_set(r, &bo); chain_run_set(r, &so); chain_run_set(r, static_cast<const sinddm_solver_opts*>(nullptr));
    r.halo_x = 16; r.sample_seeds = reinterpret_cast<const uint64_t*>(dev);
    CHECK(r.solver_q == q && r.solver_hist == hist && chain_check(r, &c) == 0 && c.ms_q == q && c.tiled && c.W == 12 + 32);
    so.q = nullptr;
    r = plain();
    chain_run_set(r, &so);
    CHECK(chain_check(r, &c) == 0 && !c.ms_q);
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails != 0;
}
"""


@pytest.mark.skipif(_host_cxx() is None, reason="no host C++ compiler")
def test_solver_checks_under_sanitizers(tmp_path):
    """The solver block's lines of chain_check in a stand-alone program with its own main, under
    -fsanitize=address,undefined: nothing is loaded into Python."""
    src, exe = tmp_path / "solver_check_main.cpp", tmp_path / "solver_check_main"
    src.write_text(SAN_MAIN)
    subprocess.check_call([_host_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "sinddm_amd", "csrc"), str(src), "-o",
                           str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- the options on the diffusion object ------------------------------------------------------------------------------------
def test_few_step_options_are_validated(c2):
    d = c2
    assert (d.sample_steps, d.sample_spacing, d.solver_order, d.eta) == (None, "t", 1, 1.0)
    assert d._few_step_cfg(0) is None
    try:
        d.sample_steps = 8
        assert d._few_step_cfg(2) == (8, "t", 1)
        d.sample_steps, d.solver_order, d.sample_spacing = [4, 5, 6, 7, None], 2, "logsnr"
        assert d._few_step_cfg(1) == (5, "logsnr", 2) and d._few_step_cfg(4) == (None, "logsnr", 2) and d._few_step_cfg(9)[0] is None
        d.resample = (2, 2)
        with pytest.raises(NotImplementedError):
            d._few_step_cfg(0)
        d.resample = None
        d.clip_guided_sampling = True
        with pytest.raises(NotImplementedError):
            d._few_step_cfg(0)
        d.clip_guided_sampling = False
        for name, val in (("sample_steps", [1, 2]), ("sample_steps", 0), ("solver_order", 3), ("sample_spacing", "snr"), ("eta", -1.0)):
            keep = getattr(d, name)
            setattr(d, name, val)
            with pytest.raises(ValueError):
                d._few_step_cfg(0)
            setattr(d, name, keep)
    finally:
        d.sample_steps, d.sample_spacing, d.solver_order, d.eta, d.resample, d.clip_guided_sampling = None, "t", 1, 1.0, None, False


def test_cli_flags():
    import main
    a = main.parse_args(["--sample_steps", "20", "--solver_order", "2", "--sample_spacing", "logsnr", "--eta", "0.5"])
    assert (a.sample_steps, a.solver_order, a.sample_spacing, a.eta) == ([20], 2, "logsnr", 0.5)
    a = main.parse_args([])
    assert (a.sample_steps, a.solver_order, a.sample_spacing, a.eta) == (None, 1, "t", 1.0)
    for bad in (["--sample_steps", "0"], ["--solver_order", "3"], ["--sample_spacing", "x"], ["--eta", "-1"]):
        with pytest.raises(SystemExit):
            main.parse_args(bad)
