"""Seed blending (sinddm_sample_chain_mix / sinddm_normal_fill_mix, `seed_mix`): sample b's N(0,1) draw for stream id j is
the fixed combination  z = sum_k w[b][k] * sinddm_normal_fill(3 H W, key[b][k], j)  of K <= 4 per-sample streams, evaluated
as  w0 * n0,  then one fused multiply-add per further seed.

  M1  the fill reduces: K = 1 with w = 1, and K = 3 with weights (1, 0, 0), are sinddm_normal_fill of the first key, bit for
      bit, n % 4 in {0, 1, 3};
  M2  the fill's arithmetic against the float64 sum of the single-seed fills: |z - ref| <= K * 2^-23 * sum_k |w_k n_k|
      (one rounding of at most 2^-24 relative per term on a partial sum bounded by sum_k |w_k n_k|, times a margin of 2);
  M3  the fill's statistics on n = 2^20 along loop_seeds(..., frames = 8, radius = 0.5): mean, variance and the correlation of
      every pair of frames inside the 6-sigma bounds of their estimators;
  M4  the blended chain is sinddm_sample_chain_solver fed opts->noise composed step-major from sinddm_normal_fill_mix, bit for
      bit, on every tail kernel and tiled; with keep + ROI maps, with a resampling jump, with a layout pull, with the multistep
      block;
  M5  K = 1, w = 1 is sinddm_sample_chain_seeds with the same seeds, bit for bit;
  M6  position does not matter: permuted rows and inputs give permuted results; one and two streams are bit-equal;
  M7  the public API on the C1 recipe: the ends of interp_seeds(A, B, 5) are the seeded samples A and B, the fused and the
      step-by-step route agree, blend_from_scale shares the coarse scales, two ranks gather the frames in order.
Shapes: the four of test_gpu_chain_guided.SHAPES (one tail kernel each; three steps incl. t = 0) and the tiled case of
test_gpu_keep.CASES, with omega = 0.3 (test_gpu_seeds._ctx) so that a wrong draw cannot hide under sigma = 1e-10.
"""
import ctypes as C
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from PIL import Image

from conftest import max_abs, rel_l2
from test_gpu_chain_guided import IDS, SHAPES, _fill, _trainer
from test_gpu_keep import CASE_IDS, CASES, _bound
from test_gpu_layout import G_CHAIN, N_CHAIN, _cells, _layout
from test_gpu_resample import JS, _jump_array, _walk
from test_gpu_seeds import BUDGET, GOLDEN, TOP, _chain_seeds, _ctx, _free_port, _seed_list
from test_gpu_solver import _sched

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _mix_rows(B, K):
    """B rows of K seeds and K unit-norm weights: both ends of the seed range, a row that is one seed alone (weights
    (1, 0, ...)), a negative weight, rows that share seeds; the rest spread over the sphere."""
    keys = [[(0x9E3779B97F4A7C15 * (b * K + k + 1)) & TOP for k in range(K)] for b in range(B)]
    keys[0][0] = 0
    keys[B - 1][K - 1] = TOP
    w = []
    for b in range(B):
        v = [math.cos(0.7 * b + 1.3 * k) + (0.25 if k == 0 else 0.0) for k in range(K)]
        nrm = math.sqrt(sum(x * x for x in v))
        w.append([x / nrm for x in v])
    if B > 1:
        w[1] = [1.0] + [0.0] * (K - 1)
    if B > 2:
        keys[2] = list(keys[1])
    return keys, w


def _dev(mix):
    return torch.tensor(mix[0], dtype=torch.int64, device=DEV), torch.tensor(mix[1], dtype=torch.float32, device=DEV)


def _fill_mix(B, n, mix, sid, guard=0):
    from sinddm_amd import _lib
    lib = _lib.load()
    kd, wd = _dev(mix)
    out = torch.full((B * n + guard,), 7.5, device=DEV)
    _lib.check(lib.sinddm_normal_fill_mix(_lib.ptr(out), B, n, _lib.ptr(kd), _lib.ptr(wd), kd.shape[1], sid, _lib.stream_ptr(DEV)),
               "sinddm_normal_fill_mix")
    torch.cuda.synchronize()
    return out


def _mix_draws(c, x0, mix, sids):
    """The contract spelled out: one slot per stream id, sample b = the blend over the EXTENDED sample; the step-major buffer
    opts->noise (or rs->noise) takes."""
    B, Cc, H, W = x0.shape
    shape = (B, Cc, H, W + 2 * c.hx)
    return torch.stack([_fill_mix(B, Cc * H * (W + 2 * c.hx), mix, sid).view(shape) for sid in sids]).contiguous()


def _run(c, x0, ts, *, mix=None, seeds=None, noise=None, jnoise=None, sid0=0, aux=False, edit=None, keep=None, jump_to=None,
         lay=None, lands=None, entry="mix", seed=0):
    """sinddm_sample_chain_mix (or _solver: the same call without the trailing block) on centre-size arguments of a
    test_gpu_keep._Ctx, extended here; the extended result.  jump_to: the walk's jump targets; lay: a layout picture (block size
    N_CHAIN, strengths G_CHAIN); lands: the multistep block of a strided run (order 2)."""
    from sinddm_amd import _lib
    from sinddm_amd.models import _aux_stream, _workspace
    lib = _lib.load()
    xa = c.ext(x0).clone()
    B, _, H, We = xa.shape
    n = len(ts)
    xb, eps, xt = torch.empty_like(xa), torch.empty_like(xa), c.ext(c.xt)
    tab = c.d._coef_table(c.s)
    coefs = (_lib.StepCoefs * n)(*([tab[t] for t in ts] if lands is None else
                                   [c.d.step_coefs_to(t, u, c.s) for t, u in zip(ts, lands)]))
    tl = (C.c_int * n)(*ts)
    ws = _workspace(DEV, lib.sinddm_workspace_bytes(c.dim, B, H, We))
    flag = C.c_int(-1)
    opts = _lib.ChainOpts()
    held = []
    if edit is not None:
        held += [c.ext(edit[0]), c.ext(edit[1])]
        opts.edit_w, opts.edit_c = _lib.ptr(held[0]), _lib.ptr(held[1])
    opts.noise = _lib.ptr(noise)
    kopts = None
    if keep is not None:
        held += [c.ext(keep[0]), c.ext(keep[1])]
        ab_tab = c.d._keep_ab_table()
        ab = (C.c_float * (2 * n))(*[float(v) for l in (lands if lands is not None else [t - 1 for t in ts]) for v in ab_tab[l + 1]])
        kopts = _lib.KeepOpts()
        kopts.mask, kopts.x0, kopts.ab = _lib.ptr(held[-2]), _lib.ptr(held[-1]), C.cast(ab, C.POINTER(C.c_float))
    ropts = None
    if jump_to is not None:
        jumps = _jump_array(c, ts, jump_to)
        ropts = _lib.ResampleOpts(C.cast(jumps, C.POINTER(_lib.JumpCoefs)), _lib.ptr(jnoise))
    lopts = None
    if lay is not None:
        h, w = _cells(H, We - 2 * c.hx, N_CHAIN)
        held += [c.ext(lay), torch.empty((B, 3, h, w), device=DEV)]
        garr = (C.c_float * n)(*[float(v) for v in G_CHAIN[:n]])
        lopts = _lib.LayoutOpts(_lib.ptr(held[-2]), N_CHAIN, C.cast(garr, C.POINTER(C.c_float)), _lib.ptr(held[-1]))
    sopts = None
    if lands is not None:
        qarr = (C.c_float * n)(*c.d._solver_q(c.s, ts, lands))
        held.append(torch.full_like(xa, float("nan")))          # (a step reads it only after one has written it)
        sopts = _lib.SolverOpts(C.cast(qarr, C.POINTER(C.c_float)), _lib.ptr(held[-1]))
    sd = torch.tensor(seeds, dtype=torch.int64, device=DEV) if seeds is not None else None
    ref = lambda o: C.byref(o) if o is not None else None
    args = [_lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
            coefs, tl, n, float(c.s), seed, sid0, c.dim, B, H, We - 2 * c.hx, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
            _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, c.hx, ref(kopts), _lib.ptr(sd), ref(ropts),
            ref(lopts), None, ref(sopts)]
    if entry == "solver":
        assert mix is None
        rc = lib.sinddm_sample_chain_solver(*args)
    else:
        mopts = None
        if mix is not None:
            kd, wd = _dev(mix)
            assert kd.shape[0] == B
            held += [kd, wd]
            mopts = _lib.MixOpts(_lib.ptr(kd), _lib.ptr(wd), kd.shape[1])
        rc = lib.sinddm_sample_chain_mix(*args, ref(mopts))
    torch.cuda.synchronize()
    assert rc == 0 and flag.value in (0, 1)
    return xb if flag.value == 1 else xa


# ---- M1: the fill reduces to the single-seed fill -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3 * 48 * 64, 3 * 9 * 11, 3 * 133 * 177], ids=["n%4=0", "n%4=1", "n%4=3"])
def test_fill_mix_of_one_seed_is_the_fill(n):
    assert n % 4 == {3 * 48 * 64: 0, 3 * 9 * 11: 1, 3 * 133 * 177: 3}[n]
    B, sid = 3, (5 << 32) | 9
    seeds = [TOP, 123456789, 0]
    out = _fill_mix(B, n, ([[v] for v in seeds], [[1.0]] * B), sid, guard=8)
    assert bool((out[B * n:] == 7.5).all())                     # (the last slice does not write past its end)
    for b in range(B):
        assert torch.equal(out[b * n:(b + 1) * n], _fill(n, seeds[b], sid)), b
    out3 = _fill_mix(B, n, ([[v, 77 + b, TOP - b] for b, v in enumerate(seeds)], [[1.0, 0.0, 0.0]] * B), sid, guard=8)
    assert torch.equal(out3, out)
    assert not torch.equal(out[:n], _fill(n, seeds[0], sid + 1))


# ---- M2: the fill's arithmetic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 4])
def test_fill_mix_against_float64_sum(K):
    B, n, sid = 4, 3 * 67 * 90 + 1, (2 << 32) | 5               # (n % 4 == 3: unaligned slices, a partial last quad)
    mix = _mix_rows(B, K)
    out = _fill_mix(B, n, mix, sid).view(B, n).double()
    w32 = torch.tensor(mix[1], dtype=torch.float32).double()    # (the weights the kernel read)
    worst = 0.0
    for b in range(B):
        terms = torch.stack([w32[b, k].item() * _fill(n, mix[0][b][k], sid).double() for k in range(K)])
        err = (out[b] - terms.sum(0)).abs()
        bound = K * 2.0 ** -23 * terms.abs().sum(0)
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (b, float(err.max()))
    print(f"K = {K}: worst |z - ref| / (K 2^-23 sum |w n|) over {B} x {n} elements: {worst:.3f}")
    assert not torch.equal(out[0], out[3])


# ---- M3: the fill's statistics --------------------------------------------------------------------------------------------------
def test_fill_mix_statistics_along_a_loop():
    from sinddm_amd.models import loop_seeds
    n, F = 1 << 20, 8
    mix = loop_seeds(11, 22, 33, F, 0.5)
    z = _fill_mix(F, n, mix, (1 << 32) | 3).view(F, n).double()
    w = torch.tensor(mix[1], dtype=torch.float64)
    mean, var = z.mean(1), z.var(1, unbiased=True)
    print("means", ["%.2e" % v for v in mean.tolist()], "variances - 1", ["%.2e" % (v - 1) for v in var.tolist()])
    assert float(mean.abs().max()) <= 6 / math.sqrt(n)
    assert float((var - 1).abs().max()) <= 6 * math.sqrt(2 / n)
    zc = (z - mean[:, None]) / z.std(1, unbiased=True)[:, None]
    corr = (zc @ zc.T / (n - 1)).cpu()
    want = w @ w.T
    off = float((corr - want).abs().max())
    print(f"largest |sample correlation - sum_k w_ik w_jk| over the {F * (F - 1) // 2} pairs: {off:.2e} (bound {6 / math.sqrt(n):.2e})")
    assert off <= 6 / math.sqrt(n)
    assert float(want[0, 4]) < 0.51 and float(want[0, 1]) > 0.9          # (the loop does move: opposite frames share only the base)


# ---- M4: the blended chain is the chain fed the blended fills -------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_blended_chain_equals_noise_buffer_of_blended_fills(cfg, dim, s, B, aux, ts, hx):
    c = _ctx(cfg, dim, s, B, hx)
    mix, sid0 = _mix_rows(B, 3), (s << 32) | 2
    y = _run(c, c.x0, ts, mix=mix, sid0=sid0, aux=aux, seed=999)                       # (`seed` is ignored)
    assert torch.isfinite(y).all()
    nz = _mix_draws(c, c.x0, mix, [sid0 + i for i in range(len(ts))])
    ref = _run(c, c.x0, ts, noise=nz, aux=aux, entry="solver")
    same = torch.equal(y, ref)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B}: blended chain vs noise buffer of blended fills max-abs "
          f"{max_abs(y.cpu(), ref.cpu()):.3e} bit-equal {same}")
    assert same
    # the tables are what is read: another weight row for the last sample moves that sample alone
    other = ([list(r) for r in mix[0]], [list(r) for r in mix[1]])
    other[1][B - 1] = [0.0, 0.6, 0.8]
    y2 = _run(c, c.x0, ts, mix=other, sid0=sid0, aux=aux)
    assert torch.equal(y2[:B - 1], y[:B - 1]) and not torch.equal(y2[B - 1], y[B - 1])
    # opts->noise wins over the block; a block with NULL keys, and no block, are sinddm_sample_chain_solver itself
    assert torch.equal(_run(c, c.x0, ts, mix=other, noise=nz, sid0=sid0, aux=aux), y)
    plain = _run(c, c.x0, ts, sid0=sid0, aux=aux, seed=77, entry="solver")
    assert torch.equal(_run(c, c.x0, ts, sid0=sid0, aux=aux, seed=77), plain)
    if aux:
        assert torch.equal(y, _run(c, c.x0, ts, mix=mix, sid0=sid0, aux=False))


@pytest.mark.parametrize("case", [0, 1, 3, 4], ids=[CASE_IDS[i] for i in (0, 1, 3, 4)])
def test_blended_chain_with_keep_and_roi_maps(case):
    cfg, dim, s, B, aux, ts, hx = CASES[case]
    c = _ctx(cfg, dim, s, B, hx)
    mix, sid0 = _mix_rows(B, 3), (s << 32) | 2
    kw = dict(aux=aux, edit=(c.ew, c.ec), keep=(c.m, c.k0))
    y = _run(c, c.x0, ts, mix=mix, sid0=sid0, **kw)
    ref = _run(c, c.x0, ts, noise=_mix_draws(c, c.x0, mix, [sid0 + i for i in range(len(ts))]), entry="solver", **kw)
    print(f"{CASE_IDS[case]} keep + ROI: max-abs {max_abs(y.cpu(), ref.cpu()):.3e}")
    assert torch.isfinite(y).all() and torch.equal(y, ref)
    assert not torch.equal(y, _run(c, c.x0, ts, mix=mix, sid0=sid0, aux=aux))          # (the maps are at work)


@pytest.mark.parametrize("case", [1, 3], ids=[CASE_IDS[1], CASE_IDS[3]])
def test_blended_chain_through_a_resampling_jump(case):
    cfg, dim, s, B, aux, _, hx = CASES[case]
    ts, jump_to = _walk(s)
    c = _ctx(cfg, dim, s, B, hx)
    mix, sid0 = _mix_rows(B, 3), (s << 32) | 2
    y = _run(c, c.x0, ts, mix=mix, sid0=sid0, aux=aux, jump_to=jump_to, keep=(c.m, c.k0))
    nz = _mix_draws(c, c.x0, mix, [sid0 + i for i in range(len(ts))])
    jn = _mix_draws(c, c.x0, mix, [sid0 + i + JS for i, l2 in enumerate(jump_to) if l2 is not None])
    ref = _run(c, c.x0, ts, noise=nz, jnoise=jn, aux=aux, jump_to=jump_to, keep=(c.m, c.k0), entry="solver")
    print(f"{CASE_IDS[case]} jump: max-abs {max_abs(y.cpu(), ref.cpu()):.3e}")
    assert torch.isfinite(y).all() and torch.equal(y, ref)
    # the jump's draw is its own stream: with the step's numbers in its place the run lands elsewhere
    assert not torch.equal(y, _run(c, c.x0, ts, noise=nz, jnoise=nz[1:2].contiguous(), aux=aux, jump_to=jump_to,
                                   keep=(c.m, c.k0), entry="solver"))


@pytest.mark.parametrize("case", [1, 3], ids=[CASE_IDS[1], CASE_IDS[3]])
def test_blended_chain_with_a_layout_pull(case):
    cfg, dim, s, B, aux, ts, hx = CASES[case]
    c = _ctx(cfg, dim, s, B, hx)
    mix, sid0 = _mix_rows(B, 3), (s << 32) | 2
    lay = _layout(c.H, c.W)
    y = _run(c, c.x0, ts, mix=mix, sid0=sid0, aux=aux, lay=lay, edit=(c.ew, c.ec))
    ref = _run(c, c.x0, ts, noise=_mix_draws(c, c.x0, mix, [sid0 + i for i in range(len(ts))]), aux=aux, lay=lay,
               edit=(c.ew, c.ec), entry="solver")
    print(f"{CASE_IDS[case]} layout: max-abs {max_abs(y.cpu(), ref.cpu()):.3e}")
    assert torch.isfinite(y).all() and torch.equal(y, ref)
    assert not torch.equal(y, _run(c, c.x0, ts, mix=mix, sid0=sid0, aux=aux, edit=(c.ew, c.ec)))


@pytest.mark.parametrize("case", [1, 3], ids=[CASE_IDS[1], CASE_IDS[3]])
def test_blended_chain_with_the_multistep_block(case):
    cfg, dim, s, B, aux, ts, hx = CASES[case]
    taus, lands = _sched(ts[0])
    c = _ctx(cfg, dim, s, B, hx)
    mix, sid0 = _mix_rows(B, 3), (s << 32) | 2
    y = _run(c, c.x0, taus, mix=mix, sid0=sid0, aux=aux, lands=lands, keep=(c.m, c.k0))
    ref = _run(c, c.x0, taus, noise=_mix_draws(c, c.x0, mix, [sid0 + i for i in range(len(taus))]), aux=aux, lands=lands,
               keep=(c.m, c.k0), entry="solver")
    print(f"{CASE_IDS[case]} multistep: max-abs {max_abs(y.cpu(), ref.cpu()):.3e}")
    assert torch.isfinite(y).all() and torch.equal(y, ref)


# ---- M5: one seed with weight 1 is the seeded chain -----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts", SHAPES, ids=IDS)
def test_one_seed_with_weight_one_is_the_seeded_chain(cfg, dim, s, B, aux, ts):
    c = _ctx(cfg, dim, s, B, 0)
    seeds, sid0 = _seed_list(B), (s << 32) | 2
    y = _run(c, c.x0, ts, mix=([[v] for v in seeds], [[1.0]] * B), sid0=sid0, aux=aux)
    ref = _chain_seeds(c, c.x0, ts, seeds, sid0=sid0, aux=aux)
    print(f"{cfg} dim {dim} s={s}: K = 1 vs sinddm_sample_chain_seeds max-abs {max_abs(y.cpu(), ref.cpu()):.3e}")
    assert torch.equal(y, ref)
    # ... and so is a wider row whose other weights are 0
    assert torch.equal(_run(c, c.x0, ts, mix=([[v, 5, 6, 7] for v in seeds], [[1.0, 0.0, 0.0, 0.0]] * B), sid0=sid0, aux=aux), ref)


# ---- M6: position does not matter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts", SHAPES, ids=IDS)
def test_position_in_the_batch_does_not_matter(cfg, dim, s, B, aux, ts):
    """The bound is the one test_gpu_seeds' G4 holds per-sample seeds to: the draws are a function of the row alone (bit for
    bit: M4), the network's kernels may round a sample differently at another position."""
    c = _ctx(cfg, dim, s, B, 0)
    mix = _mix_rows(B, 3)
    perm = [(5 * b + 3) % B for b in range(B)] if B == 16 else [2, 0, 3, 1]
    assert sorted(perm) == list(range(B)) and all(p != b for b, p in enumerate(perm))
    y = _run(c, c.x0, ts, mix=mix, sid0=2, aux=aux)
    xt = c.xt
    if xt is not None:
        c.xt = xt[perm].contiguous()
    yp = _run(c, c.x0[perm].contiguous(), ts, mix=([mix[0][p] for p in perm], [mix[1][p] for p in perm]), sid0=2, aux=aux)
    c.xt = xt
    err, bound = max_abs(yp.cpu(), y[perm].cpu()), _bound(y)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} B={B} two streams={aux}: permuted batch vs permuted result max-abs {err:.3e} "
          f"(bound {bound:.3e}) bit-equal {torch.equal(yp, y[perm])}")
    assert err <= bound
    assert max_abs(yp.cpu(), y.cpu()) > 1e-2                    # (the permutation did move the samples)
    ya = _run(c, c.x0, ts, mix=mix, sid0=2, aux=not aux)        # the two-stream guarantee: identical with and without
    assert torch.equal(y, ya)


# ---- M7: the public API ---------------------------------------------------------------------------------------------------------
A, Bs, FRAMES = 5, 8, 5


@pytest.fixture(scope="module")
def c1(golden, tmp_path_factory):
    from sinddm_amd.models import interp_seeds
    tr, meta = _trainer(golden, tmp_path_factory.mktemp("mix_c1"))
    em = tr.ema_model
    kw = dict(custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    em.draw_log = []
    frames = tr.sample_scales(batch_size=FRAMES, seed_mix=interp_seeds(A, Bs, FRAMES), **kw)
    log, em.draw_log = em.draw_log, None
    assert em.seed_mix is None and em.sample_seeds is None      # put back after the call
    return dict(tr=tr, meta=meta, kw=kw, frames=frames, log=log)


def test_interpolation_ends_are_the_seeded_samples(c1):
    from sinddm_amd.models import noise_stream_id
    tr, frames, log = c1["tr"], c1["frames"], c1["log"]
    assert [e[0] for e in log] == ["init", "chain_mix", "renoise", "chain_mix", "renoise", "chain_mix"]
    assert [e[1] for e in log if e[0] == "chain_mix"] == [0, 1, 2]
    for e in log:                                               # in noise: bit for bit
        if e[0] in ("init", "renoise"):
            z = e[3]
            assert torch.equal(z[0].reshape(-1), _fill(z[0].numel(), A, noise_stream_id(e[1], e[0])))
            assert torch.equal(z[FRAMES - 1].reshape(-1), _fill(z[0].numel(), Bs, noise_stream_id(e[1], e[0])))
            assert not torch.equal(z[2], z[0])
    ends = [tr.sample_scales(batch_size=1, seeds=[v], **c1["kw"]) for v in (A, Bs)]
    for s in range(len(frames)):
        errs = [rel_l2(frames[s][0].cpu(), ends[0][s][0].cpu()), rel_l2(frames[s][FRAMES - 1].cpu(), ends[1][s][0].cpu())]
        step = [rel_l2(frames[s][b].cpu(), frames[s][b + 1].cpu()) for b in range(FRAMES - 1)]
        print(f"scale {s}: frame 0 / frame {FRAMES - 1} vs seeds {A} / {Bs} alone, rel-L2 {['%.2e' % e for e in errs]} (budget "
              f"{BUDGET:.0e}); neighbouring frames {['%.2e' % e for e in step]}")
        assert max(errs) <= BUDGET
        assert min(step) > 1e-2                                 # (every frame is another image)
    with pytest.raises(ValueError):
        tr.sample_scales(batch_size=4, seed_mix=([[1, 2]] * 5, [[1.0, 0.0]] * 5), **c1["kw"])
    with pytest.raises(ValueError):
        tr.sample_scales(batch_size=2, seeds=[1, 2], seed_mix=([[1, 2]] * 2, [[1.0, 0.0]] * 2), **c1["kw"])
    assert tr.ema_model.seed_mix is None


def test_blend_from_scale_shares_the_coarse_scales(c1):
    from sinddm_amd.models import loop_seeds, mix_from_scale
    tr, S = c1["tr"], 1
    outs = tr.sample_scales(batch_size=4, seed_mix=mix_from_scale(loop_seeds(17, 18, 19, 4, 0.5), S, 3), **c1["kw"])
    pairs = list(itertools.combinations(range(4), 2))
    for s in range(S):
        err = max(max_abs(outs[s][a].cpu(), outs[s][b].cpu()) for a, b in pairs)
        print(f"scale {s} (below blend_from_scale): the four frames agree pairwise to max-abs {err:.3e} (bound {_bound(outs[s]):.3e})")
        assert err <= _bound(outs[s])
    near = [min(max_abs(outs[s][a].cpu(), outs[s][b].cpu()) for a, b in pairs) for s in range(S, 3)]
    print("later scales: the nearest pair of frames differs by max-abs", ["%.3e" % v for v in near])
    assert max(near) > 1e-2


@pytest.mark.parametrize("case", [0, 3, 4], ids=[CASE_IDS[0], CASE_IDS[3], CASE_IDS[4]])
def test_fused_route_equals_stepwise_route_with_a_blend(case):
    """`_run_steps` with ROI guidance: the chain call against the step-by-step route, which fills each step's draw through
    sinddm_normal_fill_mix -- over the extended size, centre kept, when tiled.  Held to the budget of the full-chain pins and to
    the max-abs bound test_gpu_seeds holds the seeded routes to."""
    cfg, dim, s, B, aux, ts, hx = CASES[case]
    c = _ctx(cfg, dim, s, B, hx)
    d, mix = c.d, _mix_rows(B, 3)
    d.roi_guided_sampling = True
    d.seed_mix = mix
    d.draw_log = []
    y = d._run_steps(c.x0.clone(), s, ts)
    assert [e[0] for e in d.draw_log] == ["chain_mix"] and d.draw_log[0][1] == s and d.draw_log[0][3] == list(ts)
    d.chain_guided = False
    d.draw_log = []
    x = d._run_steps(c.x0.clone(), s, ts)
    assert [e[0] for e in d.draw_log] == ["step"] * len(ts)
    d.draw_log = None
    err, bound, rel = max_abs(y.cpu(), x.cpu()), _bound(x), rel_l2(y.cpu(), x.cpu())
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B}: blended fused route vs stepwise route max-abs {err:.3e} "
          f"(bound {bound:.3e}) rel-L2 {rel:.2e} (budget {BUDGET:.0e})")
    assert err <= bound and rel <= BUDGET
    d.chain_guided = True                                       # ... and the fused route is the direct call
    assert torch.equal(y, c.centre(_run(c, c.x0, ts, mix=mix, sid0=(s << 32) | 2, aux=True, edit=(c.ew, c.ec))))
    d.seed_mix = (mix[0][:-1], mix[1][:-1])
    with pytest.raises(ValueError):
        d._run_steps(c.x0.clone(), s, ts)
    d.seed_mix, d.sample_seeds = mix, _seed_list(B)
    with pytest.raises(ValueError):
        d._run_steps(c.x0.clone(), s, ts)


def _rank(rank, world, port, tmp, q):
    """One rank of a two-process run on one device (gloo; tests/test_gpu_dist_sample.py): the blended sample_scales."""
    import torch.distributed as td
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet, interp_seeds
        from sinddm_amd.synth import closed_form_state_dict
        from sinddm_amd.trainer import MultiscaleTrainer
        dev = "cuda:0"
        with open(os.path.join(GOLDEN, "g11_img_scales.json")) as f:
            meta = json.load(f)["C1"]
        pyr = np.load(os.path.join(GOLDEN, "c1_pyramid.npz"))
        folder = os.path.join(tmp, f"r{rank}", "balloons") + "/"
        for key in pyr.files:
            os.makedirs(folder + key, exist_ok=True)
            Image.fromarray(pyr[key]).save(folder + key + "/balloons.png")
        net = SinDDMNet(dim=32, multiscale=True, device=dev).to(dev)
        net.load_state_dict(closed_form_state_dict(32))
        sizes = [tuple(s) for s in meta["sizes"]]
        d = MultiScaleGaussianDiffusion(net, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"], image_sizes=sizes,
                                        timesteps=20, train_full_t=True, scale_losses=meta["rescale_losses"], loss_factor=1,
                                        loss_type="l1", device=dev, reblurring=True, omega=0).to(dev)
        tr = MultiscaleTrainer(d, folder=folder, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"],
                               image_sizes=sizes, train_batch_size=2, train_num_steps=1,
                               results_folder=os.path.join(tmp, f"res{rank}"), device=dev)
        torch.manual_seed(1234 + rank)                          # (as main.py does per rank: must not matter)
        outs = tr.sample_scales(batch_size=FRAMES, seed_mix=interp_seeds(A, Bs, FRAMES), custom_t_list=d.num_timesteps_ideal[1:],
                                save_images=False)
        q.put((rank, "ok", [o.cpu().numpy() for o in outs]))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "ERR " + repr(e) + traceback.format_exc(), None))
    finally:
        td.destroy_process_group()


def test_two_ranks_gather_the_frames_in_order(c1, tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] == "ok", r[1]
    for a, b in zip(res[0][2], res[1][2]):
        assert a.shape[0] == FRAMES and np.array_equal(a, b)    # every rank holds the same gathered batch
    for s, (got, ref) in enumerate(zip(res[0][2], c1["frames"])):
        errs = [rel_l2(got[b], ref[b].cpu()) for b in range(FRAMES)]
        print(f"scale {s}: two ranks (3 + 2 frames) vs one process ({FRAMES} frames), rel-L2 per frame {['%.2e' % e for e in errs]} "
              f"(budget {BUDGET:.0e})")
        assert max(errs) <= BUDGET                              # the same frames in the same order
