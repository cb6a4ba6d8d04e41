"""GPU: one network evaluation does what its plan (forward_plan, csrc/fwd_plan.h) says.

The plan is read through sinddm_debug_forward_plan at the device's CU count (test_fwd_plan_host.py checks its structure on the
CPU).  Three things are held against it on tiny shapes: the launches the profiler counts, the workspace the evaluation accepts,
and -- because the chain and the stepwise route now read one fuse_tail -- that a three-step sinddm_sample_chain equals the same
steps taken one at a time through sinddm_net_forward + sinddm_reverse_step, bit for bit.
reference: none (launch counts and scratch layout are the library's own business; the numbers are gated elsewhere)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from sinddm_amd.synth import hash_randn
from test_fwd_plan_host import TINY, launch_counts, plan
from test_gpu_routes import FP32, INFER, _launched, _weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E_WORKSPACE = -3
_ids = lambda k: f"dim{k[0] & 0xFFFF}{'_fp32' if k[0] & FP32 else ''}_{k[1]}x{k[2]}x{k[3]}"
COUNT_SHAPES = sorted(TINY) + [(dim | (FP32 if fp32 else 0), B, H, W) for dim, fp32, B, H, W, _ in INFER if (dim, B, H, W) not in TINY]
# the padded fused tail, the plain fused tail under the head, the fused tail on the final conv, the unfused tail
CHAIN_SHAPES = [(160, 2, 9, 11), (160, 1, 20, 20), (20, 2, 8, 10), (20, 2, 9, 11)]


def _forward(L, lib, da, B, H, W, ws_bytes, out=None):
    p, pk, _ = _weights(L, lib, da & 0xFFFF)
    x = (hash_randn((B, 3, H, W), 900 + W) * 0.9).to(DEV)
    out = torch.empty_like(x) if out is None else out
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    rc = lib.sinddm_net_forward(L.ptr(p), L.ptr(pk), L.ptr(x), None, 100, 2.0, L.ptr(out), da, B, H, W, ws.data_ptr(), ws_bytes,
                                L.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("key", COUNT_SHAPES, ids=_ids)
def test_launch_counts_are_the_plans(key):
    from sinddm_amd import _lib as L
    lib = L.load()
    da, B, H, W = key
    pl = plan(lib, da, 0, B, H, W, ncu=0)
    assert pl["ncu"] == torch.cuda.get_device_properties(DEV).multi_processor_count
    L.check(lib.sinddm_prof_begin(), "sinddm_prof_begin")
    rc, out = _forward(L, lib, da, B, H, W, pl["ws_bytes"])
    n1x1 = C.c_int64(-1)
    L.check(lib.sinddm_prof_end3(2, None, C.byref(n1x1), None, None, 0), "sinddm_prof_end3")
    wino, direct = _launched(L, lib)
    want = launch_counts(pl)
    print(f"routes {pl['routes']}: launched {(wino, n1x1.value, direct)}, planned {want}")
    assert rc == 0 and (wino, n1x1.value, direct) == want
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("key", sorted(TINY), ids=_ids)
def test_workspace_is_the_plans_core_bytes(key):
    from sinddm_amd import _lib as L
    lib = L.load()
    da, B, H, W = key
    pl = plan(lib, da, 0, B, H, W, ncu=0)
    assert 0 < pl["core_bytes"] <= pl["ws_bytes"] == lib.sinddm_workspace_bytes(da, B, H, W)
    rc_full, full = _forward(L, lib, da, B, H, W, pl["ws_bytes"])
    rc_core, core = _forward(L, lib, da, B, H, W, pl["core_bytes"])
    assert rc_full == 0 and rc_core == 0 and torch.isfinite(full).all()
    assert torch.equal(core, full)
    # one byte less: a host refusal before any launch
    sentinel = torch.full((B, 3, H, W), 7.5, device=DEV)
    rc, out = _forward(L, lib, da, B, H, W, pl["core_bytes"] - 1, out=sentinel.clone())
    assert rc == E_WORKSPACE and torch.equal(out, sentinel)


def _ddpm_coefs(L, ts, T=20):
    """sinddm_step_coefs of plain DDPM posterior steps (mode 0, clipped) on a linear beta schedule of T steps."""
    beta = np.linspace(1e-3, 0.2, T)
    ac = np.cumprod(1.0 - beta)
    acp = np.concatenate([[1.0], ac[:-1]])
    var = beta * (1.0 - acp) / (1.0 - ac)
    out = (L.StepCoefs * len(ts))()
    for c, t in zip(out, ts):
        c.mode, c.clip = 0, 1
        c.sqrt_recip_ac_t, c.sqrt_recipm1_ac_t = float(np.sqrt(1.0 / ac[t])), float(np.sqrt(1.0 / ac[t] - 1.0))
        c.coef1_t = float(beta[t] * np.sqrt(acp[t]) / (1.0 - ac[t]))
        c.coef2_t = float((1.0 - acp[t]) * np.sqrt(1.0 - beta[t]) / (1.0 - ac[t]))
        c.sigma = float(np.sqrt(var[t])) if t > 0 else 0.0
    return out


@pytest.mark.parametrize("key", CHAIN_SHAPES, ids=_ids)
def test_chain_equals_the_steps_taken_one_at_a_time(key):
    """the chain and the stepwise route share their numbers -- on every kind of last launch."""
    from sinddm_amd import _lib as L
    lib = L.load()
    dim, B, H, W = key
    pl = plan(lib, dim, 0, B, H, W, ncu=0)
    assert (pl["padded"], pl["head"], pl["fuse_tail"]) == {(160, 2, 9, 11): (1, 1, 1), (160, 1, 20, 20): (0, 1, 1),
                                                           (20, 2, 8, 10): (0, 0, 1), (20, 2, 9, 11): (0, 0, 0)}[key]
    p, pk, _ = _weights(L, lib, dim)
    ts, seed, sid0, scale = [2, 1, 0], 77001 + W, 5, 1.0
    coefs, tl = _ddpm_coefs(L, ts), (C.c_int * 3)(*ts)
    x0 = (hash_randn((B, 3, H, W), 640 + H) * 0.8).to(DEV)
    ws = torch.empty(pl["ws_bytes"], dtype=torch.uint8, device=DEV)
    st = L.stream_ptr(DEV)
    xa, xb, eps, flag = x0.clone(), torch.empty_like(x0), torch.empty_like(x0), C.c_int(-1)
    L.check(lib.sinddm_sample_chain(L.ptr(p), L.ptr(pk), L.ptr(xa), L.ptr(xb), L.ptr(eps), None, coefs, tl, 3, scale, seed, sid0,
                                    dim, B, H, W, ws.data_ptr(), ws.numel(), st, C.byref(flag)), "sinddm_sample_chain")
    torch.cuda.synchronize()
    chain = xb if flag.value == 1 else xa
    x, nxt, z = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
    for i, t in enumerate(ts):
        L.check(lib.sinddm_net_forward(L.ptr(p), L.ptr(pk), L.ptr(x), None, t, scale, L.ptr(eps), dim, B, H, W, ws.data_ptr(),
                                       ws.numel(), st), "sinddm_net_forward")
        L.check(lib.sinddm_normal_fill(L.ptr(z), z.numel(), seed, sid0 + i, st), "sinddm_normal_fill")
        L.check(lib.sinddm_reverse_step(L.ptr(x), L.ptr(eps), None, L.ptr(z), L.ptr(nxt), C.byref(coefs[i]), x.numel(), st),
                "sinddm_reverse_step")
        x, nxt = nxt, x
    torch.cuda.synchronize()
    assert torch.isfinite(chain).all() and not torch.equal(chain, x0)
    diff = (chain - x).abs().max().item()
    print(f"dim {dim} {B}x{H}x{W}: chain vs stepwise max-abs {diff:.3e}")
    assert torch.equal(chain, x)
