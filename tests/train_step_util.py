"""What the GPU tests of the training step's options share (tests/test_gpu_tile_train.py, tests/test_gpu_train_mask.py,
tests/test_gpu_train_step.py): the C1 diffusion object on He-normal weights, the inputs, one p_losses + backward, the recorded
step of the "nothing changes when off" tests -- and sentinels / counters on the LIBRARY's entries.  `_lib.load()` returns the
one cached CDLL and the Python side looks an entry up per call, so an attribute set on it is what every route calls: the tests
pin which kernels ran, whatever the Python code above them looks like."""
import torch

from oracle import sinddm_oracle as O
from sinddm_amd.synth import hash_randn, he_state_dict

DEV = "cuda:0"
# the five entries a training step chooses among (train_step.TrainStep.q_entry / .loss_entry)
STEP_ENTRIES = ("sinddm_q_sample", "sinddm_q_sample_wrap", "sinddm_l1_loss_fwd_bwd", "sinddm_l1_loss_crop_fwd_bwd",
                "sinddm_l1_loss_weighted_fwd_bwd")


def sched_and_diffusion(golden, dim, loss_type="l1"):
    from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet
    meta = golden("g11_img_scales.json")["C1"]
    net = SinDDMNet(dim=dim, multiscale=True, device=DEV).to(DEV)
    sd = he_state_dict(dim)
    net.load_state_dict(sd)
    d = MultiScaleGaussianDiffusion(net, n_scales=meta["n_scales"], scale_factor=meta["scale_factor"],
                                    image_sizes=[tuple(v) for v in meta["sizes"]], timesteps=meta["T"], train_full_t=True,
                                    scale_losses=meta["rescale_losses"], loss_factor=1, loss_type=loss_type, device=DEV,
                                    reblurring=True, omega=0).to(DEV)
    sched = O.make_schedule(meta["T"], meta["n_scales"], meta["rescale_losses"], 1, train_full_t=True)
    return net, d, sd, sched


def inputs(B, H, W, key):
    """(x_start, x_orig, noise, t): an image-like pair in [-1, 1], N(0,1) noise, a different t per sample."""
    x_start = hash_randn((B, 3, H, W), key).mul(0.5).clamp(-1, 1)
    x_orig = hash_randn((B, 3, H, W), key + 1).mul(0.5).clamp(-1, 1)
    noise = hash_randn((B, 3, H, W), key + 2)
    t = torch.tensor([(7 + 24 * b) % 100 for b in range(B)])
    return x_start, x_orig, noise, t


def step(net, d, x_start, x_orig, noise, t, s):
    """p_losses + backward on the GPU: (loss as a float, {name: grad on the CPU})."""
    net.bind_grads()
    net.flat_grads.zero_()
    kw = dict(x_orig=x_orig.to(DEV)) if s > 0 else {}
    loss = d.p_losses(x_start.to(DEV), t.to(DEV), s, noise=noise.to(DEV), **kw)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()}


def recorded_step(monkeypatch, net, d, x_start, x_orig, noise, t, s, never, why):
    """One step with everything that is reproducible run to run recorded: the loss, the network's input (x_noisy) and output,
    the gradient handed to the network's backward -- and the flat gradient buffer.  While it runs, a call of any library entry
    named in `never` raises AssertionError(why)."""
    from sinddm_amd import _lib

    def refuse(*a, **k):
        raise AssertionError(why)

    rec = {}

    def hook(mod, args, out):
        rec["x_noisy"], rec["eps"] = args[0].detach().clone(), out.detach().clone()
        out.register_hook(lambda g: rec.__setitem__("grad_eps", g.detach().clone()))

    h = net.register_forward_hook(hook)
    try:
        with monkeypatch.context() as m:                                       # (undone on exit)
            for name in never:
                m.setattr(_lib.load(), name, refuse)
            rec["loss"], _ = step(net, d, x_start, x_orig, noise, t, s)
    finally:
        h.remove()
    rec["flat_grads"] = net.flat_grads.detach().cpu().clone()
    rec["named"] = {n: (p.grad.data_ptr() - net.flat_grads.data_ptr()) // 4 for n, p in net.named_parameters()}
    rec["numel"] = {n: p.numel() for n, p in net.named_parameters()}
    return rec


def count_entries(m, names=STEP_ENTRIES):
    """Wraps the library entries `names` in counting pass-through functions through the monkeypatch context `m`; returns the
    dict {name: calls}, filled as they are called."""
    from sinddm_amd import _lib
    lib, calls = _lib.load(), {}

    def wrap(name, fn):
        def counted(*a):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a)
        return counted

    for name in names:
        m.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls
