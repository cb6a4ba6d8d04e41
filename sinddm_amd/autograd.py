"""torch.autograd glue: the training forward/backward of SinDDMNet and the L1 loss run in the HIP
library; autograd only carries the (B,3,H,W) gradient between them and exposes the parameter
gradients as the `.grad` views of the flat gradient buffer (so `loss.backward()` and optimizers keep
their usual semantics -- reference trainer.py:200-209, functions.py:97-102)."""
from __future__ import annotations

import torch

from . import _lib


# generation counter of the shared training workspace per device: a second training forward before the first
# backward() would silently overwrite the first graph's saved activations, so backward checks its stamp
_WS_GEN = {}


class _NetTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, net, t, scale):
        from .models import _workspace
        lib = _lib.load()
        x = x.contiguous()
        B, C, H, W = x.shape
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        out = torch.empty_like(x)
        packed = net.packed_weights()
        nbytes = lib.sinddm_train_workspace_bytes(net.dim, B, H, W)
        ws = _workspace(x.device, nbytes, tag="train")
        _lib.check(lib.sinddm_net_forward_train(_lib.ptr(net.flat_params), _lib.ptr(packed), _lib.ptr(x), _lib.ptr(t),
                                                0, float(scale), _lib.ptr(out), net.dim_arg, B, H, W, ws.data_ptr(),
                                                ws.numel(), _lib.stream_ptr(x.device)), "sinddm_net_forward_train")
        key = ws.data_ptr()
        _WS_GEN[key] = _WS_GEN.get(key, 0) + 1
        ctx.ws_gen = (key, _WS_GEN[key])
        ctx.net, ctx.ws, ctx.shape = net, ws, (B, H, W)
        ctx.save_for_backward(x)
        ctx.need_gx = x.requires_grad
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        net = ctx.net
        (x,) = ctx.saved_tensors
        B, H, W = ctx.shape
        key, gen = ctx.ws_gen
        if ctx.ws.data_ptr() != key or _WS_GEN.get(key) != gen:
            raise _lib.SinddmError("the saved activations of this graph were overwritten by a later training forward "
                                   "(one live SinDDMNet graph per device: call backward() before the next forward)")
        grad_out = grad_out.contiguous()
        gx = torch.empty_like(x) if ctx.need_gx else None
        packed = net.packed_weights()
        packed_bwd = net.packed_weights_bwd()
        net.bind_grads()
        _lib.check(lib.sinddm_net_backward(_lib.ptr(net.flat_params), _lib.ptr(packed), _lib.ptr(packed_bwd),
                                           _lib.ptr(x), _lib.ptr(grad_out), _lib.ptr(net.flat_grads),
                                           _lib.ptr(gx) if gx is not None else None, net.dim_arg, B, H, W,
                                           ctx.ws.data_ptr(), ctx.ws.numel(), _lib.stream_ptr(x.device)),
                   "sinddm_net_backward")
        return gx, None, None, None, None


def net_forward_train(net, x, t, scale):
    """Forward that saves activations; parameter grads are accumulated straight into net.flat_grads by
    the backward kernels.  `anchor` is a dummy differentiable input so autograd schedules backward()
    even when x itself does not require grad (the usual training case)."""
    if not x.is_cuda:
        raise _lib.SinddmError("SinDDMNet needs a ROCm device tensor: there is no CPU fallback")
    anchor = net._autograd_anchor()
    return _NetTrainFn.apply(x, anchor, net, t, scale)


def l1_entry(halo, weighted: bool, rect: bool = False) -> str:
    """The library entry of the fused L1 loss: the rectangle kernel under per-sample rectangles (crop training), else the
    weighted kernel under a map, else the cropping one under a halo, else the plain mean.  The ONE owner of the rule: `_L1Fn`
    launches by it, `train_step.TrainStep` reports it."""
    if rect:
        return "sinddm_l1_loss_rect_fwd_bwd"
    if weighted:
        return "sinddm_l1_loss_weighted_fwd_bwd"
    return "sinddm_l1_loss_crop_fwd_bwd" if halo[0] or halo[1] else "sinddm_l1_loss_fwd_bwd"


class _L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, noise, eps, weight, inv_norm, halo):
        lib = _lib.load()
        noise = noise.contiguous()
        eps = eps.contiguous()
        hy, hx = int(halo[0]), int(halo[1])
        name = l1_entry((hy, hx), weight is not None)
        if name != "sinddm_l1_loss_fwd_bwd":               # (the plain mean takes any two tensors of one size)
            if weight is not None and noise.dim() != 4:
                raise _lib.SinddmError(f"l1_loss: noise must be (B,C,H,W) under a weight map, got {tuple(noise.shape)}")
            H, W = int(noise.shape[-2]), int(noise.shape[-1])
            if tuple(eps.shape) != (*noise.shape[:-2], H + 2 * hy, W + 2 * hx):
                raise _lib.SinddmError(f"l1_loss: eps {tuple(eps.shape)} is not noise {tuple(noise.shape)} extended by the halo "
                                       f"{(hy, hx)}")
        if weight is not None:
            if tuple(weight.shape) != (H, W) or weight.dtype != torch.float32 or weight.device != eps.device:
                raise _lib.SinddmError(f"l1_loss: the weight map must be a {(H, W)} fp32 tensor on {eps.device}, got "
                                       f"{tuple(weight.shape)} {weight.dtype} on {weight.device}")
            weight = weight.contiguous()
        loss = torch.zeros((), dtype=torch.float32, device=eps.device)
        g = torch.empty_like(eps)                          # the kernels write the zeros of the halo and of the holes themselves
        head, st = (_lib.ptr(noise), _lib.ptr(eps)), _lib.stream_ptr(eps.device)
        if weight is not None:
            args = (*head, _lib.ptr(weight), _lib.ptr(loss), _lib.ptr(g), int(noise.shape[0]), int(noise.shape[1]), H, W, hy, hx,
                    float(inv_norm), 1.0, st)
        elif hy or hx:
            args = (*head, _lib.ptr(loss), _lib.ptr(g), noise.numel() // (H * W), H, W, hy, hx, 1.0, st)
        else:
            args = (*head, _lib.ptr(loss), _lib.ptr(g), eps.numel(), 1.0, st)
        _lib.check(getattr(lib, name)(*args), name)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (g,) = ctx.saved_tensors
        # d loss / d eps = -sign(noise - eps) / N (times w / sum w under a map), scaled by the upstream scalar (e.g.
        # 1/grad_accumulate); its shape is eps's: exactly 0 on the halo and where w == 0
        return None, g * grad_loss, None, None, None


class _L1RectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, noise, eps, weight, inv_norm, windows, rects):
        lib = _lib.load()
        name = l1_entry((0, 0), weight is not None, True)
        noise = noise.contiguous()
        eps = eps.contiguous()
        if noise.dim() != 4 or noise.shape != eps.shape:
            raise _lib.SinddmError(f"l1_loss: noise {tuple(noise.shape)} and eps {tuple(eps.shape)} must be one (B,C,h,w) shape "
                                   f"under rectangles")
        B, Cc, h, w = (int(v) for v in noise.shape)
        for tab, cols, what in ((rects, 4, "rects"), (windows, 2, "windows")):
            if tab is None and what == "windows" and weight is None:
                continue
            if tab is None or tuple(tab.shape) != (B, cols) or tab.dtype != torch.int32 or tab.device != eps.device:
                raise _lib.SinddmError(f"l1_loss: {what} must be an int32 {(B, cols)} table on {eps.device}")
        Hm = Wm = 0
        if weight is not None:
            if weight.dim() != 2 or weight.dtype != torch.float32 or weight.device != eps.device or weight.shape[0] < h \
                    or weight.shape[1] < w:
                raise _lib.SinddmError(f"l1_loss: the weight map must be an fp32 (H,W) >= {(h, w)} tensor on {eps.device}, got "
                                       f"{tuple(weight.shape)} {weight.dtype} on {weight.device}")
            weight = weight.contiguous()
            Hm, Wm = int(weight.shape[0]), int(weight.shape[1])
        loss = torch.zeros((), dtype=torch.float32, device=eps.device)
        g = torch.empty_like(eps)                          # the kernel writes the zeros outside the rectangles itself
        _lib.check(getattr(lib, name)(_lib.ptr(noise), _lib.ptr(eps), _lib.ptr(weight),
                                      _lib.ptr(windows.contiguous()) if windows is not None else None,
                                      _lib.ptr(rects.contiguous()), _lib.ptr(loss), _lib.ptr(g), B, Cc, h, w, Hm, Wm,
                                      float(inv_norm), 1.0, _lib.stream_ptr(eps.device)), name)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (g,) = ctx.saved_tensors
        return None, g * grad_loss, None, None, None, None


def l1_loss(noise, eps, halo=(0, 0), weight=None, inv_norm=None, windows=None, rects=None):
    """mean(|noise - eps|)  (reference models.py:594) -- and the two losses of the training options, one fused kernel each:
    with a `halo` = (halo_y, halo_x), `eps` is the network's output on the image extended by its wrapped halo and the mean is
    taken over its centre (tileable training); with a `weight` -- the (H,W) fp32 map w >= 0 shared by samples and channels --
    the loss is sum(w |noise - centre(eps)|) * inv_norm, `inv_norm` = 1 / (B C sum w) from the caller, and where w == 0 nothing
    is read (masked training).  With `rects` -- an int32 (B,4) device table (y_lo, y_hi, x_lo, x_hi) -- noise and eps are
    window-size (B,C,h,w) tensors, the loss is inv_norm * the sum over every sample's rectangle, and `weight`, if any, is the
    FULL-image map read at the int32 (B,2) origins `windows` (crop training; no halo)."""
    if rects is not None:
        if halo[0] or halo[1]:
            raise _lib.SinddmError("l1_loss: rectangles and a halo do not go together")
        return _L1RectFn.apply(noise, eps, weight, inv_norm, windows, rects)
    return _L1Fn.apply(noise, eps, weight, inv_norm, halo)
