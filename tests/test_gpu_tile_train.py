"""Tileable training on the GPU: wrap-around borders in the training step (MultiScaleGaussianDiffusion.train_tile).

No convolution kernel knows circular padding.  p_losses writes x_noisy extended by a wrapped halo of SINDDM_TILE_HALO = 16 pixels
(sinddm_q_sample_wrap), runs the zero-padded training forward / backward on the extended image and takes the loss on the centre
(sinddm_l1_loss_crop_fwd_bwd): the loss and every parameter gradient are those of the circularly padded network
(tests/test_tile_train_host.py proves the construction in float64; tests/tile_train_util.py is that network).  Here:

  1. sinddm_q_sample_wrap = sinddm_q_sample followed by sinddm_wrap_halo, bit for bit;
  2. sinddm_l1_loss_crop_fwd_bwd: zeros on the halo of a NaN-filled buffer, the centre bit-equal to sinddm_l1_loss_fwd_bwd;
  3. p_losses + backward against the circular reference (float64, CPU), and the zero-padded oracle is measurably another step;
  4. the step commutes with toroidal shifts of its inputs;
  5. the loss types 'l2' and 'l1_pred_img';
  6. train_tile = (False, False) is the untouched step: bit for bit wherever the step is reproducible at all.
The shapes are the smallest at which each path can go wrong: a halo wider than the image (5x7), the one-float and the 16-byte
kernels (W % 4), one axis against both, B > 1 with per-sample t, s = 0 and s > 0."""
import pytest
import torch

from conftest import rel_l2
from fullrank_util import oracle_p_losses_autograd
from sinddm_amd.synth import hash_randn
from tile_train_util import WRAPS, circular_p_losses_autograd, halo_of
from train_step_util import DEV, inputs as _inputs, recorded_step, sched_and_diffusion as _sched_and_diffusion, step as _step

pytestmark = pytest.mark.gpu

# (B, H, W, halo_y, halo_x) of tests 1 and 2.  5x7: the halo wraps more than once, one-float kernels (sinddm_q_sample's too:
# 3*5*7 is odd); 9x32, 12x20, 8x36: the 16-byte kernels, one axis and both.  The fifth: sinddm_q_sample takes its 16-byte
# kernel (3*4*7 % 4 == 0) while the fused kernel takes its one-float path (W = 7) -- the rounding must follow the former.
SHAPES = [(2, 5, 7, 16, 16), (3, 9, 32, 0, 16), (1, 12, 20, 16, 0), (2, 8, 36, 16, 16), (2, 4, 7, 16, 16)]


# ---- 1: sinddm_q_sample_wrap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,hy,hx", SHAPES, ids=lambda v: str(v))
def test_q_sample_wrap_is_q_sample_then_wrap_halo(golden, B, H, W, hy, hx):
    from sinddm_amd import _lib
    lib = _lib.load()
    _, d, _, _ = _sched_and_diffusion(golden, 16)
    x0, xo, nz, t = (v.to(DEV) for v in _inputs(B, H, W, 40 + W))
    gamma_row = d.gammas[1].reshape(-1).contiguous()
    assert 0.0 < float(gamma_row[7]) < 1.0                                    # the mix is a real one at the first sample's t
    He, We = H + 2 * hy, W + 2 * hx
    for with_orig in (False, True):
        for t_dev, t_host in ((t, 0), (None, 31)):
            two = d._wrap_pad(d._q_sample_impl(x0, t_dev, t_host, nz, x_orig=xo if with_orig else None,
                                               gamma_row=gamma_row if with_orig else None), hy, hx)
            guard = 8
            big = torch.full((guard + B * 3 * He * We + guard,), float("nan"), device=DEV)
            rc = lib.sinddm_q_sample_wrap(_lib.ptr(x0), _lib.ptr(xo) if with_orig else None, _lib.ptr(nz),
                                          big.data_ptr() + 4 * guard, _lib.ptr(d.sqrt_alphas_cumprod),
                                          _lib.ptr(d.sqrt_one_minus_alphas_cumprod), _lib.ptr(gamma_row) if with_orig else None,
                                          _lib.ptr(t_dev) if t_dev is not None else None, t_host, B, 3, H, W, hy, hx,
                                          _lib.stream_ptr(DEV))
            torch.cuda.synchronize()
            assert rc == 0
            one = big[guard:-guard].view(B, 3, He, We)
            assert torch.equal(one, two), (with_orig, t_host)
            assert bool(big[:guard].isnan().all()) and bool(big[-guard:].isnan().all())
    # the Python route of p_losses is this call
    assert torch.equal(d._q_sample_impl(x0, t, 0, nz, x_orig=xo, gamma_row=gamma_row, halo=(hy, hx)),
                       d._wrap_pad(d._q_sample_impl(x0, t, 0, nz, x_orig=xo, gamma_row=gamma_row), hy, hx))


# ---- 2: sinddm_l1_loss_crop_fwd_bwd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,hy,hx", SHAPES[:4], ids=lambda v: str(v))
def test_l1_loss_crop(B, H, W, hy, hx):
    from sinddm_amd import _lib
    lib = _lib.load()
    He, We = H + 2 * hy, W + 2 * hx
    noise = hash_randn((B, 3, H, W), 70 + W).to(DEV)
    eps_ext = hash_randn((B, 3, He, We), 71 + W).to(DEV)
    centre = eps_ext[:, :, hy:hy + H, hx:hx + W]
    centre[0, 0, 0, :3] = noise[0, 0, 0, :3]                                  # exact ties: sign(0) = 0
    centre[-1, 2, H - 1, W - 2:] = noise[-1, 2, H - 1, W - 2:]
    crop = centre.contiguous()
    st = _lib.stream_ptr(DEV)
    loss_ref = torch.zeros((), device=DEV)
    g_ref = torch.empty_like(crop)
    _lib.check(lib.sinddm_l1_loss_fwd_bwd(_lib.ptr(noise), _lib.ptr(crop), _lib.ptr(loss_ref), _lib.ptr(g_ref), crop.numel(), 0.5,
                                          st), "sinddm_l1_loss_fwd_bwd")
    guard = 8
    big = torch.full((guard + eps_ext.numel() + guard,), float("nan"), device=DEV)
    loss = torch.zeros((), device=DEV)
    _lib.check(lib.sinddm_l1_loss_crop_fwd_bwd(_lib.ptr(noise), _lib.ptr(eps_ext), _lib.ptr(loss), big.data_ptr() + 4 * guard,
                                               B * 3, H, W, hy, hx, 0.5, st), "sinddm_l1_loss_crop_fwd_bwd")
    torch.cuda.synchronize()
    g = big[guard:-guard].view(B, 3, He, We)
    assert not bool(g.isnan().any())                                          # every element was written
    assert torch.equal(g[:, :, hy:hy + H, hx:hx + W], g_ref)
    assert int((g_ref == 0).sum()) == 5                                       # the planted ties, and only those
    halo = g.clone()
    halo[:, :, hy:hy + H, hx:hx + W] = 0.0
    assert torch.equal(halo, torch.zeros_like(halo))                          # (-0.0 == 0.0: "exactly 0" is the value)
    assert int((g != 0).sum()) == crop.numel() - 5
    assert bool(big[:guard].isnan().all()) and bool(big[-guard:].isnan().all())
    assert abs(float(loss) - float(loss_ref)) <= 1e-6 * abs(float(loss_ref))
    # the autograd wrapper: the same numbers, scaled by the upstream gradient
    from sinddm_amd.autograd import l1_loss
    e = eps_ext.clone().requires_grad_(True)
    out = l1_loss(noise, e, (hy, hx))
    (out * 0.5).backward()
    assert abs(float(out) - float(loss_ref)) <= 1e-6 * abs(float(loss_ref))
    assert torch.equal(e.grad, g)


# ---- 3: gradients against the circular reference ----------------------------------------------------------------------------------
GRAD_CASES = [(16, 1, 5, 7, "xy", 0), (32, 3, 9, 33, "x", 2), (80, 2, 14, 40, "y", 2), (160, 2, 21, 37, "xy", 2)]


@pytest.mark.parametrize("dim,B,H,W,wrap,s", GRAD_CASES, ids=lambda v: str(v))
def test_p_losses_gradients_vs_circular_reference(golden, dim, B, H, W, wrap, s):
    """Loss < 1e-5 relative, all 52 parameter gradients < 2e-4 rel-L2 against p_losses_circular under float64 autograd on the
    CPU (the tolerances tests/test_gpu_train.py::test_net_backward_vs_oracle_autograd holds these kernels to at these sizes);
    and the ZERO-padded oracle's gradients are more than 1e-2 away from the circular ones in at least one tensor, so the
    comparison can tell the two steps apart."""
    net, d, sd, sched = _sched_and_diffusion(golden, dim)
    x_start, x_orig, noise, t = _inputs(B, H, W, 100 + dim)
    d.train_tile = WRAPS[wrap]
    loss, grads = _step(net, d, x_start, x_orig, noise, t, s)
    xo = x_orig if s > 0 else None
    l_ref, g_ref = circular_p_losses_autograd(sched, sd, x_start, xo, t, s, noise, WRAPS[wrap])
    l_zero, g_zero = oracle_p_losses_autograd(sched, sd, x_start, xo, t, s, noise, "l1", torch.float64)
    errs = {k: rel_l2(grads[k], g_ref[k]) for k in g_ref}
    apart = {k: rel_l2(g_zero[k], g_ref[k]) for k in g_ref}
    print(f"[dim {dim} B{B} {H}x{W} {wrap} s={s}] loss {loss:.7g} vs {l_ref:.7g} ({abs(loss - l_ref) / abs(l_ref):.1e}); worst "
          f"gradient {max(errs.values()):.2e} ({max(errs, key=errs.get)}); zero-padded vs circular {min(apart.values()):.3f} .. "
          f"{max(apart.values()):.3f}")
    assert len(errs) == 52
    assert abs(loss - l_ref) < 1e-5 * abs(l_ref)
    for k, e in errs.items():
        assert e < 2e-4, (k, e)
    assert max(apart.values()) > 1e-2


# ---- 4: shift equivariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,B,H,W,wrap", [(32, 3, 9, 33, "x"), (32, 2, 12, 20, "xy")], ids=lambda v: str(v))
def test_step_commutes_with_toroidal_shifts(golden, dim, B, H, W, wrap):
    """A property only a truly periodic step has: rolling x_start, x_orig and noise by (3, 5) along the wrapped axes changes
    neither the loss nor any parameter gradient -- beyond 4e-4 rel-L2, twice test 3's bound (triangle inequality through the
    common reference).  The plain step on the same inputs moves by far more in at least one tensor."""
    net, d, sd, sched = _sched_and_diffusion(golden, dim)
    x_start, x_orig, noise, t = _inputs(B, H, W, 300 + W)
    wr = WRAPS[wrap]
    shifts, dims = zip(*[(sh, ax) for sh, ax, on in ((3, 2, wr[0]), (5, 3, wr[1])) if on])
    roll = lambda v: torch.roll(v, shifts, dims).contiguous()
    d.train_tile = wr
    l0, g0 = _step(net, d, x_start, x_orig, noise, t, 2)
    l1, g1 = _step(net, d, roll(x_start), roll(x_orig), roll(noise), t, 2)
    errs = {k: rel_l2(g1[k], g0[k]) for k in g0}
    d.train_tile = (False, False)
    _, p0 = _step(net, d, x_start, x_orig, noise, t, 2)
    _, p1 = _step(net, d, roll(x_start), roll(x_orig), roll(noise), t, 2)
    plain = max(rel_l2(p1[k], p0[k]) for k in p0)
    print(f"[dim {dim} B{B} {H}x{W} {wrap}] rolled vs not: loss {abs(l1 - l0) / abs(l0):.1e}, worst gradient "
          f"{max(errs.values()):.2e} ({max(errs, key=errs.get)}); the plain step: {plain:.3f}")
    assert abs(l1 - l0) < 4e-4 * abs(l0)
    for k, e in errs.items():
        assert e < 4e-4, (k, e)
    assert plain > 1e-2


# ---- 5: the other loss types ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lt", ["l2", "l1_pred_img"])
def test_other_loss_types(golden, lt):
    """'l2' / 'l1_pred_img' slice the centre out of the extended x_recon (torch ops; the slice's backward zero-fills the halo):
    dim 16, B = 2, 9x12, both axes wrapped, s = 0 and s = 2 (t[0] > 0: the mixed target of 'l1_pred_img')."""
    net, d, sd, sched = _sched_and_diffusion(golden, 16, loss_type=lt)
    d.train_tile = (True, True)
    x_start, x_orig, noise, t = _inputs(2, 9, 12, 500)
    for s in (0, 2):
        loss, grads = _step(net, d, x_start, x_orig, noise, t, s)
        l_ref, g_ref = circular_p_losses_autograd(sched, sd, x_start, x_orig if s > 0 else None, t, s, noise, (True, True), lt)
        errs = {k: rel_l2(grads[k], g_ref[k]) for k in g_ref}
        print(f"[{lt} s={s}] loss {loss:.7g} vs {l_ref:.7g}; worst gradient {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
        assert abs(loss - l_ref) < 1e-5 * abs(l_ref)
        for k, e in errs.items():
            assert e < 2e-4, (lt, s, k, e)


# ---- 6: nothing changes when off ------------------------------------------------------------------------------------------------------
def _recorded_step(golden, touch, x_start, x_orig, noise, t, s, monkeypatch):
    """One plain step on a fresh diffusion object (train_step_util.recorded_step), during which the two library entries of
    the tiled route refuse to run."""
    net, d, _, _ = _sched_and_diffusion(golden, 16)
    if touch:
        d.train_tile = (False, False)
    return recorded_step(monkeypatch, net, d, x_start, x_orig, noise, t, s, ("sinddm_q_sample_wrap", "sinddm_l1_loss_crop_fwd_bwd"),
                         "a kernel of the tiled route ran with train_tile off")


@pytest.mark.parametrize("s", [0, 2])
def test_off_is_the_untouched_step(golden, monkeypatch, s):
    """train_tile = (False, False) set explicitly against a diffusion object whose attribute was never touched (dim 16, B = 2,
    7x12: 504 elements, so the loss is the sum of two workgroups' partial sums, which commutes).  Neither library entry
    of the tiled route (sinddm_q_sample_wrap, sinddm_l1_loss_crop_fwd_bwd) is called, and the loss, x_noisy, the network's
    output and the gradient handed to its backward are bit-equal.

    The flat gradient buffer is NOT compared bit for bit: the backward kernels accumulate with fp32 atomics whose order
    varies from run to run, on the untouched object against itself too.  Measured: 8 fresh objects running this same plain
    step at dim 16 on 5x7 (B = 1), 7x12 and 9x12, at dim 32 on 9x33 and at dim 160 on 21x37, s = 0 and 2 -- at no shape did
    a second run reproduce the first's buffer (20 to 31 of the 52 tensors differ, worst tensor here 1.2e-7 rel-L2), and at
    9x12, where the loss is three workgroups' sum, the loss itself came out equal in 4 runs of 8;
    tests/test_gpu_train.py::test_weight_gradients_reproducible_run_to_run states the same and bounds it.  The buffer is
    held to that test's bound, 2e-6 rel-L2 per tensor, and the untouched object run twice is held to the same bound."""
    x_start, x_orig, noise, t = _inputs(2, 7, 12, 600)
    a = _recorded_step(golden, False, x_start, x_orig, noise, t, s, monkeypatch)
    a2 = _recorded_step(golden, False, x_start, x_orig, noise, t, s, monkeypatch)
    b = _recorded_step(golden, True, x_start, x_orig, noise, t, s, monkeypatch)
    for other, what in ((a2, "untouched, again"), (b, "train_tile = (False, False)")):
        assert other["loss"] == a["loss"], what
        for k in ("x_noisy", "eps", "grad_eps"):
            assert torch.equal(other[k], a[k]), (what, k)
        worst = 0.0
        for n, off in a["named"].items():
            sl = slice(off, off + a["numel"][n])
            worst = max(worst, rel_l2(other["flat_grads"][sl], a["flat_grads"][sl]))
            assert rel_l2(other["flat_grads"][sl], a["flat_grads"][sl]) < 2e-6, (what, n)
        print(f"[s={s}] {what}: flat gradients bit-equal {torch.equal(other['flat_grads'], a['flat_grads'])}, worst tensor "
              f"{worst:.1e} rel-L2")
    assert float(a["flat_grads"].abs().sum()) > 0
