"""Shared by tests/test_tile_train_host.py and tests/test_gpu_tile_train.py: the training step of the CIRCULARLY padded network,
restated in torch.

Tileable training (MultiScaleGaussianDiffusion.train_tile) extends x_noisy by a wrapped halo of SINDDM_TILE_HALO pixels, runs
the zero-padded network on the extended image and takes the loss on the centre.  The claim is that the loss AND every
parameter gradient are then those of the network whose convolutions pad circularly on the wrapped axes (and with zeros on the
others) -- what the reference gets by setting padding_mode='circular' on its nn.Conv2d's.  This file is that network, written
without the halo: `conv_block_circular` / `net_forward_circular` restate the oracle's conv_block / net_forward with an explicit
F.pad in front of every padded convolution; the condition path, the GELU and x_noisy are the oracle's own functions.  The oracle
(oracle/sinddm_oracle.py) is not edited, and nothing is patched: the functions are differentiable as they stand, in the dtype of
their inputs."""
import torch
import torch.nn.functional as F

from oracle import sinddm_oracle as O

HALO = 16          # SINDDM_TILE_HALO

WRAPS = {"x": (False, True), "y": (True, False), "xy": (True, True)}     # name -> (wrap_y, wrap_x)


def pad_wrap(x, p, wrap):
    """`p` pixels of padding on both sides of the last two axes: circular where `wrap` = (wrap_y, wrap_x) is set, zeros
    elsewhere."""
    py, px = (p if wrap[0] else 0), (p if wrap[1] else 0)
    if py or px:
        x = F.pad(x, (px, px, py, py), mode="circular")
    if p - py or p - px:
        x = F.pad(x, (p - px, p - px, p - py, p - py))
    return x


def conv_block_circular(sd, name, x, cond, wrap):
    """O.conv_block (reference SinDDM/models.py:69-80) with every padded convolution padded by pad_wrap."""
    cin = x.shape[1]
    h = F.conv2d(pad_wrap(x, 2, wrap), sd[f"{name}.ds_conv.weight"], sd[f"{name}.ds_conv.bias"], groups=cin)
    h = h + O.block_condition(sd, name, cond)[:, :, None, None]
    u = F.conv2d(pad_wrap(h, 1, wrap), sd[f"{name}.net.0.weight"], sd[f"{name}.net.0.bias"])
    o = F.conv2d(pad_wrap(O.gelu(u), 1, wrap), sd[f"{name}.net.2.weight"], sd[f"{name}.net.2.bias"])
    if f"{name}.res_conv.weight" in sd:
        r = F.conv2d(x, sd[f"{name}.res_conv.weight"], sd[f"{name}.res_conv.bias"])
    else:
        r = x
    return o + r


def net_forward_circular(sd, x, t, scale, wrap):
    """O.net_forward (reference SinDDM/models.py:134-151) of the circularly padded blocks."""
    cond = O.cond_vector(sd, t, scale)
    for name in ("l1", "l2", "l3", "l4"):
        x = conv_block_circular(sd, name, x, cond, wrap)
    return F.conv2d(x, sd["final_conv.0.weight"], sd["final_conv.0.bias"])


def p_losses_circular(sched, sd, x_start, t, s, noise, x_orig, wrap, loss_type="l1"):
    """O.p_losses (reference SinDDM/models.py:578-611) with the circularly padded network: the L1 loss main.py selects, or
    one of the two other loss types."""
    eps = net_forward_circular(sd, O.p_losses_inputs(sched, x_start, t, s, noise, x_orig), t, s, wrap)
    if loss_type == "l1":
        return (noise - eps).abs().mean()
    if loss_type == "l2":
        return F.mse_loss(noise, eps)
    if loss_type == "l1_pred_img":
        if int(s) > 0:
            if int(t[0]) > 0:
                g = O.extract(sched["gammas"][s - 1].reshape(-1), t - 1)
                x_mix_prev = g * x_start + (1 - g) * x_orig
            else:
                x_mix_prev = x_orig
        else:
            x_mix_prev = x_start
        return (x_mix_prev - eps).abs().mean()
    raise NotImplementedError(loss_type)


def wrap_pad(t, hy, hx):
    """(..., H, W) -> (..., H + 2 hy, W + 2 hx) by modulo indexing (a halo may be wider than the image)."""
    H, W = t.shape[-2], t.shape[-1]
    iy = torch.arange(-hy, H + hy, device=t.device) % H
    ix = torch.arange(-hx, W + hx, device=t.device) % W
    return t[..., iy[:, None], ix[None, :]]


def halo_of(wrap):
    return (HALO if wrap[0] else 0, HALO if wrap[1] else 0)


def autograd_in(dtype, fn, sd, *tensors):
    """fn(params, *tensors) -> scalar, under autograd with everything in `dtype` (the oracle builds its embeddings in the
    default dtype): (value, {name: grad})."""
    torch.set_default_dtype(dtype)
    try:
        p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        cast = [a.to(dtype) if torch.is_tensor(a) and a.is_floating_point() else a for a in tensors]
        val = fn(p, *cast)
        val.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return val.detach(), {k: v.grad for k, v in p.items()}


def sched_in(sched, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sched.items()}


def circular_p_losses_autograd(sched, sd, x_start, x_orig, t, s, noise, wrap, loss_type="l1", dtype=torch.float64):
    """p_losses_circular under autograd in `dtype`: (loss as a float, {name: grad})."""
    sc = sched_in(sched, dtype)
    if x_orig is None:
        fn = lambda p, xs, nz: p_losses_circular(sc, p, xs, t, s, nz, None, wrap, loss_type)
        val, g = autograd_in(dtype, fn, sd, x_start, noise)
    else:
        fn = lambda p, xs, nz, xo: p_losses_circular(sc, p, xs, t, s, nz, xo, wrap, loss_type)
        val, g = autograd_in(dtype, fn, sd, x_start, noise, x_orig)
    return float(val), g
