"""Shared by tests/test_weight_fill_host.py, tests/test_gpu_fullrank.py and tests/test_oracle_golden.py: float64 references of
the network, the mutations that show what a parity test can see, and the regions of an image where an edge bug lives.

Why: the closed-form fill of sinddm_amd/synth.py gives every conv weight, reshaped to (C_out, C_in k k), rank 2.  A network of
such weights forgets most of its input (tests/test_weight_fill_host.py measures it), so a test that judges a kernel loads
`he_state_dict` instead.  The oracle (oracle/sinddm_oracle.py) is not edited: the spatial mutations patch the one function it
convolves with, for the duration of a `with` block, as tests/tile_util.py does."""
import contextlib
from unittest import mock

import torch
import torch.nn.functional as F

from oracle import sinddm_oracle as O


# ---- float64 references -----------------------------------------------------------------------------------------------------
def net_forward_f64(sd, x, t, scale):
    """The oracle's network in float64 (the conditioning vector comes from the fp32 oracle: it is not what is tested)."""
    cond = O.cond_vector(sd, t, scale).double()
    sd64 = {k: v.double() for k, v in sd.items()}
    h = x.double()
    for name in ("l1", "l2", "l3", "l4"):
        h = O.conv_block(sd64, name, h, cond)
    return F.conv2d(h, sd64["final_conv.0.weight"], sd64["final_conv.0.bias"])


def oracle_autograd(sd, x, t, scale, gy, dtype):
    """y, grad_x and the 52 parameter gradients of O.net_forward under torch autograd, everything in `dtype`."""
    torch.set_default_dtype(dtype)
    try:
        s = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        xc = x.to(dtype).clone().requires_grad_(True)
        y = O.net_forward(s, xc, t, scale)
        y.backward(gy.to(dtype))
    finally:
        torch.set_default_dtype(torch.float32)
    return y.detach(), xc.grad, {k: v.grad for k, v in s.items()}


def klass(name):
    """The classes of parameter gradients whose fp32 error differs in kind: the condition path's and the depthwise bias's are
    plain sums over all pixels (tests/test_gpu_train.py)."""
    if ".mlp." in name or "time_mlp" in name or "time_reshape" in name or name.endswith("ds_conv.bias"):
        return "cond_path"
    return "weight" if name.endswith("weight") else "bias"


BLOCK_KEYS = ("ds_conv.weight", "ds_conv.bias", "net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias",
              "res_conv.weight", "res_conv.bias")


def block_autograd(sd, name, x, cond_bias, gy, dtype):
    """One SinDDMConvBlock (reference SinDDM/models.py:69-80) with the per-sample condition given as `cond_bias` (B, C_in),
    under autograd in `dtype`: y, grad_x, grad of cond_bias, {key: grad} for the block's conv / depthwise tensors."""
    cin = x.shape[1]
    xr = x.to(dtype).clone().requires_grad_(True)
    cbr = cond_bias.to(dtype).clone().requires_grad_(True)
    w = {k: sd[f"{name}.{k}"].to(dtype).clone().requires_grad_(True) for k in BLOCK_KEYS if f"{name}.{k}" in sd}
    h = F.conv2d(xr, w["ds_conv.weight"], w["ds_conv.bias"], padding=2, groups=cin) + cbr[:, :, None, None]
    o = F.conv2d(F.gelu(F.conv2d(h, w["net.0.weight"], w["net.0.bias"], padding=1)), w["net.2.weight"], w["net.2.bias"], padding=1)
    o = o + (F.conv2d(xr, w["res_conv.weight"], w["res_conv.bias"]) if "res_conv.weight" in w else xr)
    o.backward(gy.to(dtype))
    return o.detach(), xr.grad, cbr.grad, {k: v.grad for k, v in w.items()}


# ---- regions -------------------------------------------------------------------------------------------------------------------
def edge_regions(H, W):
    """(name, bool mask (H, W)) of the places a whole-image norm dilutes: the outer ring of 4 pixels, the last tile column
    (columns from 32 (ceil(W / 32) - 1) on: the widest tile of any 3x3 kernel here) and the last band of 8 rows."""
    ring = torch.ones(H, W, dtype=torch.bool)
    if H > 8 and W > 8:
        ring[4:-4, 4:-4] = False
    col = torch.zeros(H, W, dtype=torch.bool)
    col[:, 32 * ((W + 31) // 32 - 1):] = True
    row = torch.zeros(H, W, dtype=torch.bool)
    row[8 * ((H + 7) // 8 - 1):, :] = True
    return [("ring4", ring), ("last_tile_column", col), ("last_row_band", row)]


# ---- mutations: what a wrong kernel would compute, made on the oracle ---------------------------------------------------------
def _swap(t, dim, i, j):
    idx = list(range(t.shape[dim]))
    idx[i], idx[j] = j, i
    return t.index_select(dim, torch.tensor(idx)).contiguous()


def _mut_transpose(sd):
    sd["l3.net.0.weight"] = sd["l3.net.0.weight"].transpose(2, 3).contiguous()


def _mut_swap_in(sd):
    sd["l3.net.2.weight"] = _swap(sd["l3.net.2.weight"], 1, 7, 24)


def _mut_swap_out(sd):
    sd["l2.net.0.weight"] = _swap(sd["l2.net.0.weight"], 0, 7, 24)
    sd["l2.net.0.bias"] = _swap(sd["l2.net.0.bias"], 0, 7, 24)


def _mut_zero_tap(sd):
    w = sd["l3.net.0.weight"].clone()
    w[:, 5, 0, 0] = 0.0
    sd["l3.net.0.weight"] = w


def _mut_truncate(sd):
    sd["l3.net.2.weight"] = (sd["l3.net.2.weight"].contiguous().view(torch.int32) & ~0x7F).view(torch.float32)


# the five weight mutations of the table: name -> function that edits a copied state dict in place
WEIGHT_MUTATIONS = {
    "transpose_taps_l3_net0": _mut_transpose,
    "swap_in_channels_7_24_l3_net2": _mut_swap_in,
    "swap_out_channels_7_24_l2_net0": _mut_swap_out,
    "zero_one_tap_one_channel_l3_net0": _mut_zero_tap,
    "truncate_l3_net2_to_16_mantissa_bits": _mut_truncate,
}


@contextlib.contextmanager
def spatial_mutation(kind, sd):
    """The oracle with ONE convolution of `sd` evaluated wrongly in space (found by the identity of its weight tensor):
    'replicate_right_l3_net0' -- the first 3x3 conv of block 3 pads its right edge by replication instead of zeros;
    'shift_dw_l2'             -- the depthwise 5x5 of block 2 reads its window one column to the right."""
    real = F.conv2d
    target = {"replicate_right_l3_net0": sd["l3.net.0.weight"], "shift_dw_l2": sd["l2.ds_conv.weight"]}[kind]

    def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if w is target and kind == "replicate_right_l3_net0":
            x = F.pad(x, (1, 0, 1, 1))
            x = torch.cat((x, x[..., -1:]), dim=-1)
            return real(x, w, b, stride, 0, dilation, groups)
        if w is target and kind == "shift_dw_l2":
            return real(F.pad(x, (1, 3, 2, 2)), w, b, stride, 0, dilation, groups)
        return real(x, w, b, stride, padding, dilation, groups)

    with mock.patch.object(O.F, "conv2d", conv2d):
        yield


SPATIAL_MUTATIONS = ("replicate_right_l3_net0", "shift_dw_l2")


def mutated_forward(sd, x, t, scale, name):
    """O.net_forward of `sd` under one mutation (fp32)."""
    if name in WEIGHT_MUTATIONS:
        s2 = dict(sd)
        WEIGHT_MUTATIONS[name](s2)
        return O.net_forward(s2, x, t, scale)
    with spatial_mutation(name, sd):
        return O.net_forward(sd, x, t, scale)


# ---- the reverse step's clip ---------------------------------------------------------------------------------------------------
def clipped_fraction(sched, x, eps, t, s, x_tilde):
    """Fraction of elements that reverse_step's clip_denoised changes at step (t, s) (oracle.reverse_step, reblurring,
    lines 'x_tm1_mix.clamp' / 'x_t_mix.clamp'): a chain test sees eps only through the elements that are NOT clipped."""
    B = x.shape[0]
    tt = torch.full((B,), int(t), dtype=torch.long)
    x0 = O.extract(sched["sqrt_recip_alphas_cumprod"], tt) * x - O.extract(sched["sqrt_recipm1_alphas_cumprod"], tt) * eps
    if int(s) == 0:
        return float((x0.abs() > 1).double().mean())
    g = sched["gammas"][s - 1].reshape(-1).clamp(0, 0.55)
    mix = (x0 - O.extract(g, tt) * x_tilde) / (1 - O.extract(g, tt))
    if t > 0:
        g1 = O.extract(g, tt - 1)
        mix = g1 * x_tilde + (1 - g1) * mix
    return float(((mix.abs() > 1) | (x0.abs() > 1)).double().mean())


# ---- the chain of tests/test_gpu_fullrank.py (its clip condition is checked in tests/test_weight_fill_host.py) ----------------
CHAIN_CFG, CHAIN_SCALE, CHAIN_TS = "C2", 1, [200, 100, 0]


def chain_inputs(B, H, W):
    """Start and x-tilde of the chain tests: amplitudes at which, with sinddm_amd.synth.HE_EPS_GAIN, fewer than a fifth of
    the elements of x_recon are clipped at the steps of CHAIN_TS."""
    from sinddm_amd.synth import hash_randn
    return hash_randn((B, 3, H, W), 61) * 0.5, (hash_randn((B, 3, H, W), 62) * 0.4).clamp(-1, 1)


# ---- G22: the reference on He weights (tests/golden/make_golden.py: g22) -------------------------------------------------------
G22_FORWARD = [(160, 37, 41, (0, 2)), (160, 24, 50, (0, 2)), (32, 67, 90, (2,))]
G22_LOSSES = [("l1", 2), ("l2", 2), ("l2", 0)]
G22_GRADS = ("final_conv.0.weight", "l2.net.0.weight", "l1.ds_conv.weight")


def g22_forward_inputs(H, W):
    from sinddm_amd.synth import hash_randn
    return hash_randn((2, 3, H, W), 2200 + W), torch.tensor([17, 503])


def g22_loss_inputs(pyr, s):
    """(x_start, x_orig or None, t, noise) of the p_losses cases, from the C1 pyramid fixture."""
    from sinddm_amd.synth import hash_randn, noise_key
    to_t = lambda a: torch.from_numpy(a.transpose(2, 0, 1).copy()).float().div(255).mul(2).sub(1)
    orig = to_t(pyr[f"scale_{s}"])[None].repeat(2, 1, 1, 1)
    recon = to_t(pyr[f"scale_{s}_recon"])[None].repeat(2, 1, 1, 1) if s > 0 else orig
    noise = hash_randn(tuple(orig.shape), noise_key("train", s, 22))
    return (recon if s > 0 else orig), (orig if s > 0 else None), torch.tensor([37, 5]), noise


def oracle_p_losses_autograd(sched, sd, x_start, x_orig, t, s, noise, loss_type, dtype):
    """O.p_losses under autograd in `dtype`: (loss, {name: grad})."""
    torch.set_default_dtype(dtype)
    try:
        p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        sc = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sched.items()}
        loss = O.p_losses(sc, p, x_start.to(dtype), t, s, noise.to(dtype),
                          x_orig=None if x_orig is None else x_orig.to(dtype), loss_type=loss_type)
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return float(loss.detach()), {k: v.grad for k, v in p.items()}
