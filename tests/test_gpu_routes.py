"""GPU: the kernels a network evaluation LAUNCHES are the ones sinddm_debug_routes predicts.

Every other test that means to exercise one kernel asserts a debug hook and then trusts that block_forward / block_backward
take the same decision.  Here one evaluation runs between sinddm_prof_begin and sinddm_prof_end3, and the profiler's launch
counts -- Winograd 3x3 launches per kernel generation (kind 1: 2 = conv_wino2, 3 = conv_wino3, 4 = conv_wino4, 8 = conv_wh)
and direct 3x3 launches (kind 3) -- are compared with the table of the hook.  The C_in = 3 kernel is not profiled and is left out
of both sides.  One shape per route; the batch is raised at the same H x W if the device's CU count asks for it.
The training test also counts the Winograd-domain weight-gradient launches (kind 4: generation 8 = wgrad_wh_kernel, 0 = the two
fp32 kernels) against sinddm_debug_wgrad_routes at the device's CU count.
reference: none (which kernel runs is the library's own business; the numbers are gated elsewhere)
"""
import ctypes as C

import pytest
import torch

from sinddm_amd.synth import closed_form_state_dict, hash_randn, net_param_shapes
from test_gpu_fullrank import _batch_for

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FP32 = 0x10000
GENS = (2, 3, 4, 8)

# (dim, fp32_convs, B, H, W, the dim -> dim route at 256 CUs)
INFER = [(160, 0, 32, 96, 128, 8), (160, 1, 32, 96, 128, 4), (160, 0, 28, 99, 130, 8), (160, 0, 16, 48, 64, 3),
         (160, 0, 1, 20, 20, 2), (80, 0, 16, 186, 248, 8), (20, 0, 4, 133, 177, 2), (10, 0, 4, 30, 30, 0)]
TRAIN = [(160, 0, 32, 96, 128, 8), (160, 1, 32, 96, 128, 4), (160, 0, 2, 21, 37, 2)]
WGRAD_WINO, WGRAD_WINO_WIDE, WGRAD_WH = 3, 4, 5
_ids = lambda c: f"dim{c[0]}{'_fp32' if c[1] else ''}_{c[2]}x{c[3]}x{c[4]}_route{c[5]}"

_W = {}


def _weights(L, lib, dim):
    """(params, packed, packed_bwd) of the closed-form network, once per width."""
    if dim not in _W:
        sd = closed_form_state_dict(dim)
        p = torch.cat([sd[k].reshape(-1).float() for k in net_param_shapes(dim)]).to(DEV).contiguous()
        pk = torch.zeros(lib.sinddm_packed_count(dim), device=DEV)
        pkb = torch.zeros(lib.sinddm_packed_bwd_count(dim), device=DEV)
        st = L.stream_ptr(DEV)
        L.check(lib.sinddm_pack_weights(L.ptr(p), L.ptr(pk), dim, st), "sinddm_pack_weights")
        L.check(lib.sinddm_pack_weights_bwd(L.ptr(p), L.ptr(pkb), dim, st), "sinddm_pack_weights_bwd")
        _W[dim] = (p, pk, pkb)
    return _W[dim]


def _predicted(lib, da, train, B, H, W):
    out = (C.c_int * 16)()
    assert lib.sinddm_debug_routes(da, train, B, H, W, out) == 0
    r = list(out)
    return {g: r.count(g) for g in GENS}, r.count(0), r


def _launched(L, lib):
    """({generation: kind-1 launches}, kind-3 launches) recorded since sinddm_prof_begin."""
    def count(kind):
        n = C.c_int64(-1)
        L.check(lib.sinddm_prof_end3(kind, None, C.byref(n), None, None, 0), "sinddm_prof_end3")
        return n.value
    wino, direct, total = {g: count(10 + g) for g in GENS}, count(3), count(1)
    L.check(lib.sinddm_prof_end3(0, None, None, None, None, 1), "sinddm_prof_end3")
    assert sum(wino.values()) == total, "a Winograd launch of a generation the routes do not know"
    return wino, direct


@pytest.mark.parametrize("case", INFER, ids=_ids)
def test_inference_launches_what_the_routes_say(case):
    from sinddm_amd import _lib as L
    lib = L.load()
    dim, fp32, B, H, W, want = case
    da = dim | (FP32 if fp32 else 0)
    B = _batch_for(lib.sinddm_debug_infer_path, da, B, H, W, want)
    p, pk, _ = _weights(L, lib, dim)
    x = (hash_randn((B, 3, H, W), 900 + W) * 0.9).to(DEV)
    out = torch.empty_like(x)
    ws = torch.empty(lib.sinddm_workspace_bytes(da, B, H, W), dtype=torch.uint8, device=DEV)
    wino, direct, r = _predicted(lib, da, 0, B, H, W)
    assert r[5] == want
    L.check(lib.sinddm_prof_begin(), "sinddm_prof_begin")
    L.check(lib.sinddm_net_forward(L.ptr(p), L.ptr(pk), L.ptr(x), None, 100, 2.0, L.ptr(out), da, B, H, W, ws.data_ptr(),
                                   ws.numel(), L.stream_ptr(DEV)), "sinddm_net_forward")
    torch.cuda.synchronize()
    got = _launched(L, lib)
    print(f"routes {r[:8]}: launched {got}, predicted {(wino, direct)}")
    assert got == (wino, direct), r
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("case", TRAIN, ids=_ids)
def test_training_launches_what_the_routes_say(case):
    from sinddm_amd import _lib as L
    lib = L.load()
    dim, fp32, B, H, W, want = case
    da = dim | (FP32 if fp32 else 0)
    B = _batch_for(lib.sinddm_debug_train_path, da, B, H, W, want)
    p, pk, pkb = _weights(L, lib, dim)
    x = (hash_randn((B, 3, H, W), 900 + W) * 0.9).to(DEV)
    gy = (hash_randn((B, 3, H, W), 901 + W) * 0.1).to(DEV)
    y, gx, gp = torch.empty_like(x), torch.empty_like(x), torch.zeros_like(p)
    ws = torch.empty(lib.sinddm_train_workspace_bytes(da, B, H, W), dtype=torch.uint8, device=DEV)
    st = L.stream_ptr(DEV)
    wino, direct, r = _predicted(lib, da, 1, B, H, W)
    assert r[5] == want
    wr = (C.c_int * 68)()
    assert lib.sinddm_debug_wgrad_routes(da, B, H, W, torch.cuda.get_device_properties(DEV).multi_processor_count, wr, 68) == 0
    wk = list(wr)[0::4]
    wgrad = (wk.count(WGRAD_WH), wk.count(WGRAD_WINO) + wk.count(WGRAD_WINO_WIDE))
    assert sum(wgrad) > 0 and (wgrad[0] > 0) == (want == 8) and (W % 4 != 0) == (WGRAD_WINO in wk), wk
    L.check(lib.sinddm_prof_begin(), "sinddm_prof_begin")
    L.check(lib.sinddm_net_forward_train(L.ptr(p), L.ptr(pk), L.ptr(x), None, 100, 2.0, L.ptr(y), da, B, H, W, ws.data_ptr(),
                                         ws.numel(), st), "sinddm_net_forward_train")
    L.check(lib.sinddm_net_backward(L.ptr(p), L.ptr(pk), L.ptr(pkb), L.ptr(x), L.ptr(gy), L.ptr(gp), L.ptr(gx), da, B, H, W,
                                    ws.data_ptr(), ws.numel(), st), "sinddm_net_backward")
    torch.cuda.synchronize()
    n48, n40 = C.c_int64(-1), C.c_int64(-1)
    L.check(lib.sinddm_prof_end3(48, None, C.byref(n48), None, None, 0), "sinddm_prof_end3")
    L.check(lib.sinddm_prof_end3(40, None, C.byref(n40), None, None, 0), "sinddm_prof_end3")
    got = _launched(L, lib)
    print(f"routes {r}: launched {got}, predicted {(wino, direct)}; weight gradients {wk}: launched {(n48.value, n40.value)}, "
          f"predicted {wgrad}")
    assert got == (wino, direct), r
    assert (n48.value, n40.value) == wgrad, wk
    assert torch.isfinite(y).all() and torch.isfinite(gx).all() and torch.isfinite(gp).all()
