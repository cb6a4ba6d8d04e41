"""Per-sample noise seeds (sinddm_sample_chain_seeds / sinddm_normal_fill_samples, `sample_seeds`): the N(0,1) draw of
element e of sample b for stream id j is element e of sinddm_normal_fill(3 H W, seed_b, j), whatever batch, position,
half-batch or rank the sample runs in.

  G1  the fill: slice b of sinddm_normal_fill_samples is sinddm_normal_fill(n, seeds[b], sid), n % 4 in {0, 1, 3};
  G2  the seeded chain is sinddm_sample_chain_keep fed the same numbers as a noise buffer, bit for bit, on every tail kernel,
      with keep + ROI maps, and tiled;
  G3  a batch of one is today's sinddm_sample_chain_ex with seed = the sample's seed, bit for bit;
  G4  position does not matter: permuted seeds and inputs give permuted results; one and two streams are bit-equal;
  G5  batch size and rank count do not matter through `sample_scales`; the fused and the step-by-step route agree;
  G6  `vary_from_scale`: same coarse scales, different fine scales, reproducible;
  G7  without seeds `_run_steps` logs the ('chain', s, seed, ...) entry with the seed torch drew.
Shapes: the four of test_gpu_chain_guided.SHAPES (one tail kernel each; three steps incl. t = 0) and the tiled case of
test_gpu_keep.CASES; the C1 recipe (dim 32, T = 20) for the public API.
"""
import ctypes as C
import itertools
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from PIL import Image

from conftest import max_abs, rel_l2
from test_gpu_chain_guided import IDS, SHAPES, _chain_ex, _fill, _setup, _trainer
from test_gpu_keep import CASE_IDS, CASES, _bound, _chain, _Ctx

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOP = (1 << 63) - 1                                             # the largest seed: the key's high word is all ones but one


def _seed_list(B):
    """B seeds: the two ends of the range, one pair of equal seeds, the rest spread over both key words."""
    out = [(0x9E3779B97F4A7C15 * (b + 1)) & TOP for b in range(B)]
    out[0] = 0
    if B > 1:
        out[1] = TOP
    if B > 3:
        out[3] = out[2]
    return out


def _dev_seeds(seeds):
    return torch.tensor(seeds, dtype=torch.int64, device=DEV)


def _chain_seeds(c, x0, ts, seeds, sid0=0, aux=False, edit=None, keep=None, noise=None, seed=0):
    """sinddm_sample_chain_seeds on centre-size arguments of a test_gpu_keep._Ctx, extended here; the extended result."""
    from sinddm_amd import _lib
    from sinddm_amd.models import _aux_stream, _workspace
    lib = _lib.load()
    xa = c.ext(x0).clone()
    B, _, H, We = xa.shape
    n = len(ts)
    xb, eps, xt = torch.empty_like(xa), torch.empty_like(xa), c.ext(c.xt)
    tab = c.d._coef_table(c.s)
    coefs = (_lib.StepCoefs * n)(*[tab[t] for t in ts])
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
        ab = (C.c_float * (2 * n))(*[float(v) for t in ts for v in ab_tab[t]])
        kopts = _lib.KeepOpts()
        kopts.mask, kopts.x0, kopts.ab = _lib.ptr(held[-2]), _lib.ptr(held[-1]), C.cast(ab, C.POINTER(C.c_float))
    sd = _dev_seeds(seeds) if seeds is not None else None
    assert sd is None or sd.numel() == B
    rc = lib.sinddm_sample_chain_seeds(
        _lib.ptr(c.net.flat_params), _lib.ptr(c.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps), _lib.ptr(xt),
        coefs, tl, n, float(c.s), seed, sid0, c.dim, B, H, We - 2 * c.hx, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV),
        _aux_stream(DEV) if aux else None, C.byref(flag), C.byref(opts), 0, c.hx,
        C.byref(kopts) if kopts is not None else None, _lib.ptr(sd))
    torch.cuda.synchronize()
    assert rc == 0 and flag.value in (0, 1)
    return xb if flag.value == 1 else xa


def _ctx(cfg, dim, s, B, hx):
    """test_gpu_keep._Ctx with omega = 0.3: the configs' omega = 0 leaves the steps of the scales above the first a sigma of
    1e-10, under which a wrong draw would hide in the rounding of all but the smallest values."""
    c = _Ctx(cfg, dim, s, B, hx)
    c.d.omega = 0.3
    if s > 0:
        assert c.d._coef_table(s)[400].sigma > 0.1
    return c


def _sample_draws(c, x0, seeds, n_steps, sid0):
    """The contract spelled out: step i, sample b = sinddm_normal_fill(3 H W, seeds[b], sid0 + i) over the EXTENDED sample;
    as the step-major buffer opts->noise takes."""
    B, Cc, H, W = x0.shape
    shape = (Cc, H, W + 2 * c.hx)
    n = Cc * H * (W + 2 * c.hx)
    return torch.stack([torch.stack([_fill(n, seeds[b], sid0 + i).view(shape) for b in range(B)])
                        for i in range(n_steps)]).contiguous()


# ---- G1: the fill ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3 * 48 * 64, 3 * 9 * 11, 3 * 133 * 177], ids=["n%4=0", "n%4=1", "n%4=3"])
def test_fill_samples_is_the_fill_per_slice(n):
    from sinddm_amd import _lib
    lib = _lib.load()
    assert n % 4 == {3 * 48 * 64: 0, 3 * 9 * 11: 1, 3 * 133 * 177: 3}[n]
    B, sid = 3, (5 << 32) | 9
    seeds = [TOP, 123456789, TOP]                               # two equal seeds, one other
    guard = 7.5
    out = torch.full((B * n + 8,), guard, device=DEV)           # (the last slice must not write past its end)
    _lib.check(lib.sinddm_normal_fill_samples(_lib.ptr(out), B, n, _lib.ptr(_dev_seeds(seeds)), sid, _lib.stream_ptr(DEV)),
               "sinddm_normal_fill_samples")
    torch.cuda.synchronize()
    assert bool((out[B * n:] == guard).all())
    sl = [out[b * n:(b + 1) * n] for b in range(B)]
    for b in range(B):
        assert torch.equal(sl[b], _fill(n, seeds[b], sid)), b
    assert torch.equal(sl[0], sl[2]) and not torch.equal(sl[0], sl[1])
    assert not torch.equal(sl[0], _fill(n, seeds[0], sid + 1))
    assert abs(float(out[:B * n].mean())) < 0.05 and abs(float(out[:B * n].std()) - 1.0) < 0.05


# ---- G2: the seeded chain is the chain fed the same numbers -------------------------------------------------------------------
@pytest.mark.parametrize("with_maps", [False, True], ids=["plain", "keep_edit"])
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts,hx", CASES, ids=CASE_IDS)
def test_seeded_chain_equals_noise_buffer_of_per_sample_fills(cfg, dim, s, B, aux, ts, hx, with_maps):
    c = _ctx(cfg, dim, s, B, hx)
    seeds, sid0 = _seed_list(B), (s << 32) | 2
    assert c.d._coef_table(s)[ts[-1]].sigma == 0.0              # the run includes a step without noise
    edit = (c.ew, c.ec) if with_maps else None
    keep = (c.m, c.k0) if with_maps else None
    y = _chain_seeds(c, c.x0, ts, seeds, sid0=sid0, aux=aux, edit=edit, keep=keep, seed=999)      # (`seed` is ignored)
    assert torch.isfinite(y).all()
    ref = _chain(c, c.x0, ts, 0, aux=aux, edit=edit, keep=keep, noise=_sample_draws(c, c.x0, seeds, len(ts), sid0))
    same = torch.equal(y, ref)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B} maps={with_maps}: seeded chain vs noise buffer of per-sample "
          f"fills max-abs {max_abs(y.cpu(), ref.cpu()):.3e} bit-equal {same}")
    assert same
    # the seeds are what is read: another seed for the last sample moves that sample alone
    other = list(seeds)
    other[B - 1] ^= 1
    y2 = _chain_seeds(c, c.x0, ts, other, sid0=sid0, aux=aux, edit=edit, keep=keep)
    assert torch.equal(y2[:B - 1], y[:B - 1]) and not torch.equal(y2[B - 1], y[B - 1])
    # opts->noise wins over the seeds; seeds = NULL is sinddm_sample_chain_keep itself
    nz = _sample_draws(c, c.x0, other, len(ts), sid0)
    assert torch.equal(_chain_seeds(c, c.x0, ts, seeds, sid0=sid0, aux=aux, edit=edit, keep=keep, noise=nz), y2)
    assert torch.equal(_chain_seeds(c, c.x0, ts, None, sid0=sid0, aux=aux, edit=edit, keep=keep, seed=77),
                       _chain(c, c.x0, ts, 77, sid0=sid0, aux=aux, edit=edit, keep=keep))
    if aux:
        assert torch.equal(y, _chain_seeds(c, c.x0, ts, seeds, sid0=sid0, aux=False, edit=edit, keep=keep))
    # equal seeds and equal inputs give equal samples (seeds[2] == seeds[3]); last: it overwrites a row of x-tilde
    xe = c.x0.clone()
    xe[3] = xe[2]
    if c.xt is not None:
        c.xt[3] = c.xt[2]
    ye = _chain_seeds(c, xe, ts, seeds, sid0=sid0, aux=aux, edit=edit, keep=keep)
    assert seeds[2] == seeds[3] and torch.equal(ye[2], ye[3]) and not torch.equal(ye[1], ye[2])


# ---- G3: a batch of one ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 3], ids=[IDS[0], IDS[3]])
def test_batch_of_one_is_chain_ex_with_that_seed(idx):
    cfg, dim, s, _, _, ts = SHAPES[idx]
    c = _ctx(cfg, dim, s, 1, 0)
    for sigma in (TOP, 424242):
        y = _chain_seeds(c, c.x0, ts, [sigma], sid0=2)
        rc, _, ref = _chain_ex(c.net, c.d, s, c.x0, c.xt, ts, sigma, 2, dim)
        assert rc == 0
        assert torch.equal(y, ref), (sigma, max_abs(y.cpu(), ref.cpu()))


# ---- G4: position does not matter --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dim,s,B,aux,ts", SHAPES, ids=IDS)
def test_position_in_the_batch_does_not_matter(cfg, dim, s, B, aux, ts):
    c = _ctx(cfg, dim, s, B, 0)
    seeds = [1000 + 17 * b for b in range(B)]
    perm = [(5 * b + 3) % B for b in range(B)] if B == 16 else [2, 0, 3, 1]
    assert sorted(perm) == list(range(B)) and all(p != b for b, p in enumerate(perm))
    y = _chain_seeds(c, c.x0, ts, seeds, sid0=2, aux=aux)
    xt = c.xt
    if xt is not None:
        c.xt = xt[perm].contiguous()
    yp = _chain_seeds(c, c.x0[perm].contiguous(), ts, [seeds[p] for p in perm], sid0=2, aux=aux)
    c.xt = xt
    err, bound = max_abs(yp.cpu(), y[perm].cpu()), _bound(y)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} B={B} two streams={aux}: permuted batch vs permuted result max-abs {err:.3e} "
          f"(bound {bound:.3e}) bit-equal {torch.equal(yp, y[perm])}")
    assert err <= bound
    assert max_abs(yp.cpu(), y.cpu()) > 1e-2                    # (the permutation did move the samples)
    if aux:                                                     # the two-stream guarantee: identical with and without
        assert torch.equal(y, _chain_seeds(c, c.x0, ts, seeds, sid0=2, aux=False))


# ---- G5: batch size, rank count and route do not matter, through the public API -----------------------------------------------
BUDGET = 1e-4               # rel-L2 per scale: the budget of the project's full-chain pins (README, test_gpu_chain_pin.py)


@pytest.fixture(scope="module")
def c1(golden, tmp_path_factory):
    tr, meta = _trainer(golden, tmp_path_factory.mktemp("seeds_c1"))
    em = tr.ema_model
    kw = dict(custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    em.draw_log = []
    four = tr.sample_scales(batch_size=4, seeds=[5, 6, 7, 8], **kw)
    log, em.draw_log = em.draw_log, None
    assert em.sample_seeds is None                              # put back after the call
    return dict(tr=tr, meta=meta, kw=kw, four=four, log=log)


def test_seeded_run_takes_one_seeded_chain_per_scale(c1):
    log = c1["log"]
    assert [e[0] for e in log] == ["init", "chain_seeds", "renoise", "chain_seeds", "renoise", "chain_seeds"]
    assert all(e[2] == [5, 6, 7, 8] for e in log if e[0] == "chain_seeds")
    assert [e[1] for e in log if e[0] == "chain_seeds"] == [0, 1, 2]
    # the init / re-noise draws are the contract's fills
    from sinddm_amd.models import noise_stream_id
    for e in log:
        if e[0] in ("init", "renoise"):
            z = e[3]
            for b, sigma in enumerate([5, 6, 7, 8]):
                assert torch.equal(z[b].reshape(-1), _fill(z[b].numel(), sigma, noise_stream_id(e[1], e[0])))


def test_batch_size_does_not_matter(c1):
    tr, four = c1["tr"], c1["four"]
    one = tr.sample_scales(batch_size=1, seeds=[7], **c1["kw"])
    two = tr.sample_scales(batch_size=2, seeds=[6, 8], **c1["kw"])
    for s in range(len(four)):
        errs = [rel_l2(one[s][0].cpu(), four[s][2].cpu()), rel_l2(two[s][0].cpu(), four[s][1].cpu()),
                rel_l2(two[s][1].cpu(), four[s][3].cpu())]
        far = min(rel_l2(four[s][a].cpu(), four[s][b].cpu()) for a, b in itertools.combinations(range(4), 2))
        print(f"scale {s}: seed 7 alone / seeds 6, 8 as a pair vs the batch of four, rel-L2 {['%.2e' % e for e in errs]} "
              f"(budget {BUDGET:.0e}); nearest pair of different seeds {far:.2e}")
        assert max(errs) <= BUDGET
        assert far > 1e4 * BUDGET * 1e-2                        # different seeds: O(1) apart (> 1e-2)
    with pytest.raises(ValueError):
        tr.sample_scales(batch_size=2, seeds=[1, 2, 3], **c1["kw"])
    with pytest.raises(ValueError):
        tr.sample_scales(batch_size=2, vary_from_scale=1, **c1["kw"])
    assert tr.ema_model.sample_seeds is None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, tmp, q):
    """One rank of a two-process run on one device (gloo; tests/test_gpu_dist_sample.py): the seeded sample_scales."""
    import torch.distributed as td
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
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
        outs = tr.sample_scales(batch_size=4, seeds=[5, 6, 7, 8], custom_t_list=d.num_timesteps_ideal[1:], save_images=False)
        q.put((rank, "ok", [o.cpu().numpy() for o in outs]))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "ERR " + repr(e) + traceback.format_exc(), None))
    finally:
        td.destroy_process_group()


def test_rank_count_does_not_matter(c1, tmp_path):
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
        assert a.shape[0] == 4 and np.array_equal(a, b)        # every rank holds the same gathered batch
    for s, (got, ref) in enumerate(zip(res[0][2], c1["four"])):
        errs = [rel_l2(got[b], ref[b].cpu()) for b in range(4)]
        print(f"scale {s}: two ranks (2 + 2 chains) vs one process (4 chains), rel-L2 per sample {['%.2e' % e for e in errs]} "
              f"(budget {BUDGET:.0e})")
        assert max(errs) <= BUDGET                              # the same images in the same order


@pytest.mark.parametrize("case", [0, 3, 4], ids=[CASE_IDS[0], CASE_IDS[3], CASE_IDS[4]])
def test_fused_route_equals_stepwise_route_with_seeds(case):
    """`_run_steps` with ROI guidance: the chain call (chain_guided) against the step-by-step route, which fills each step's
    draw through sinddm_normal_fill_samples -- over the extended size, centre kept, when tiled."""
    cfg, dim, s, B, aux, ts, hx = CASES[case]
    c = _ctx(cfg, dim, s, B, hx)
    d = c.d
    d.roi_guided_sampling = True
    d.sample_seeds = _seed_list(B)
    d.draw_log = []
    y = d._run_steps(c.x0.clone(), s, ts)
    assert [e[0] for e in d.draw_log] == ["chain_seeds"] and d.draw_log[0][1:] == (s, _seed_list(B), list(ts))
    d.chain_guided = False
    d.draw_log = []
    x = d._run_steps(c.x0.clone(), s, ts)
    assert [e[0] for e in d.draw_log] == ["step"] * len(ts)
    d.draw_log = None
    err, bound = max_abs(y.cpu(), x.cpu()), _bound(x)
    print(f"{cfg} dim {dim} s={s} {c.H}x{c.W} halo_x={hx} B={B}: seeded fused route vs seeded stepwise route max-abs {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound
    # ... and the fused route is the direct call
    d.chain_guided = True
    assert torch.equal(y, c.centre(_chain_seeds(c, c.x0, ts, _seed_list(B), sid0=(s << 32) | 2, aux=True, edit=(c.ew, c.ec))))
    d.sample_seeds = _seed_list(B)[:-1]
    with pytest.raises(ValueError):
        d._run_steps(c.x0.clone(), s, ts)


# ---- G6: variations ----------------------------------------------------------------------------------------------------------
def test_variations_share_coarse_scales_and_differ_in_fine_ones(c1):
    tr = c1["tr"]
    S = 1                                                       # the middle one of C1's three scales
    outs = tr.sample_scales(batch_size=4, seeds=[17, 17, 17, 17], vary_from_scale=S, **c1["kw"])
    again = tr.sample_scales(batch_size=4, seeds=[17, 17, 17, 17], vary_from_scale=S, **c1["kw"])
    assert len(outs) == 3 and all(torch.equal(a, b) for a, b in zip(outs, again))
    pairs = list(itertools.combinations(range(4), 2))
    for s in range(S):
        err = max(max_abs(outs[s][a].cpu(), outs[s][b].cpu()) for a, b in pairs)
        print(f"scale {s} (below vary_from_scale): the four samples agree pairwise to max-abs {err:.3e} "
              f"(bound {_bound(outs[s]):.3e})")
        assert err <= _bound(outs[s])
    near = min(max_abs(outs[-1][a].cpu(), outs[-1][b].cpu()) for a, b in pairs)
    print(f"finest scale: the nearest pair of variations differs by max-abs {near:.3e}")
    assert near > 1e-2
    assert tr.ema_model.sample_seeds is None


# ---- G7: unseeded is untouched -----------------------------------------------------------------------------------------------
def test_unseeded_after_seeded_logs_the_torch_seed():
    cfg, dim, s, B, aux, ts = SHAPES[0]
    net, d, H, W, x0, xt, ew, ec = _setup(cfg, dim, s, B)
    d.sample_seeds = _seed_list(B)
    d.draw_log = []
    d._run_steps(x0.clone(), s, ts)
    assert [e[0] for e in d.draw_log] == ["chain_seeds"]
    d.sample_seeds = None
    torch.manual_seed(11)
    seed_api = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
    torch.manual_seed(11)
    d.draw_log = []
    y = d._run_steps(x0.clone(), s, ts)
    log, d.draw_log = d.draw_log, None
    assert log == [("chain", s, seed_api, list(ts))]
    rc, _, ref = _chain_ex(net, d, s, x0, None, ts, seed_api, 0, dim, aux=True)
    assert rc == 0 and torch.equal(y, ref)
