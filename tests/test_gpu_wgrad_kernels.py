"""GPU: the six weight-gradient kernels ONE LAUNCH AT A TIME (sinddm_debug_wgrad), under the grids of 64-, 256- and 304-CU
devices and the device's own, against the plain float64 reference of tests/wgrad_util.py.

C1 (test_exact): integer-valued operands on which every kernel must return the float64 reference bit for bit, whatever the
    order of its atomics (the argument is in wgrad_util.py, its premises are tested in test_wgrad_kernels_host.py), at the
    smallest shapes that reach each edge: one pixel, fewer pixel tiles than splits, one column past a tile, ragged channel
    slabs, C_in = 15 | 16, the direct 3x3 slab kernel with and without a staging slab and as the fallback of a launch table
    that does not fit, binary16 launches with an all-zero sample and with a sample 2^12 larger than the other.  A second call
    into the same gradient must double it exactly (the hook ADDS).
C2 (test_rounding): white operands (dout scaled as an L1-mean loss hands it over): gw and gb in rel-L2 against float64 <= K = 3 x
    the error of an fp32 evaluation on the CPU, per tensor, and gw per slab of the kernel with the factor doubled
    (tests/test_gpu_fullrank.py); the binary16 kernel additionally <= 1.5 x max(that yardstick, the library's wide fp32 Winograd
    kernel), the conv_wh gate.  gw's fp32 evaluation is wgrad_ref(float32); gb's is the worse of torch's pairwise sum and a
    serial loop over the pixels (wgrad_util.noise_gate says why).
Every case names the kernel it means to test and asserts that the plan took it.
reference SinDDM/models.py:63,65,67 (nn.Conv2d; the gradient is torch autograd's, restated in wgrad_util.wgrad_ref)"""
import ctypes as C

import pytest
import torch

from wgrad_util import (K, K_WH, KERNEL_NAMES, NCUS, SLAB3, WINO_WIDE, c1_cases, c1_inputs, c2_cases, c2_id, case_id,
                        exact_failures, gb_serial, noise_gate, plan, wgrad_ref, white_inputs)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from sinddm_amd import _lib
    return _lib, _lib.load()


def _device_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _run(lib, taps, ci, co, ncu, scr, amax, dout_d, x_d, gw_d, gb_d):
    """One launch, ADDED into gw_d / gb_d; returns plan_out."""
    L, _ = _lib()
    B, _, H, W = dout_d.shape
    nbytes = lib.sinddm_debug_wgrad_scratch_bytes(taps, ci, co, B)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = (C.c_int * 4)()
    rc = lib.sinddm_debug_wgrad(taps, ci, co, B, H, W, ncu, scr, amax, L.ptr(dout_d), L.ptr(x_d), L.ptr(gw_d), L.ptr(gb_d),
                                scratch.data_ptr(), nbytes, out, L.stream_ptr(DEV))
    L.check(rc, "sinddm_debug_wgrad")
    torch.cuda.synchronize(DEV)
    return tuple(out)


def _grids(lib, taps, ci, co, B, H, W, scr, amax, ncus):
    """The compute-unit counts whose grids differ (plan and, for the Winograd kernels, launch table): ncu -> the counts it
    stands for.  0 = the device's own count, passed as such."""
    seen = {}
    for n in ncus:
        key = plan(lib, taps, ci, co, B, H, W, scr, amax, n if n > 0 else _device_cus())
        seen.setdefault(key, []).append(n)
    return {v[0]: v for v in seen.values()}


@pytest.mark.parametrize("case", c1_cases(), ids=case_id)
def test_exact(case):
    kernel, taps, ci, co, B, H, W, scr, amax, variant = case
    _, lib = _lib()
    dout, x = c1_inputs(case)
    w64, b64 = wgrad_ref(dout, x, taps, torch.float64)
    dout_d, x_d = dout.to(DEV), x.to(DEV)
    k = 3 if taps == 9 else 1
    for ncu, stands_for in _grids(lib, taps, ci, co, B, H, W, scr, amax, (0,) + NCUS).items():
        gw = torch.zeros(co, ci, k, k, device=DEV)
        gb = torch.zeros(co, device=DEV)
        for times in (1, 2):
            got = _run(lib, taps, ci, co, ncu, scr, amax, dout_d, x_d, gw, gb)
            assert got[0] == kernel, (KERNEL_NAMES[kernel], got)
            assert got == plan(lib, taps, ci, co, B, H, W, scr, amax, ncu if ncu > 0 else _device_cus())[:4]
            assert got[3] == int(kernel > SLAB3 or (kernel == SLAB3 and scr))
            fails = exact_failures(gw.cpu(), gb.cpu(), w64, b64, kernel, times)
            assert not fails, (case_id(case), f"ncu {stands_for} plan {got} call {times}: (slab, wrong elements, first index)", fails)


_YARD = {}


def _c2_case(c):
    """Inputs, both references and the serial fp32 bias gradient of a C2 case, computed once (the binary16 cases share them
    with their fp32 twins)."""
    _, taps, ci, co, B, H, W, amax, sd, sx = c
    key = (taps, ci, co, B, H, W, sd, sx)
    if key not in _YARD:
        dout, x = white_inputs((B, ci, co, H, W), 8100 + 7 * ci + co + W)
        dout, x = dout * sd, x * sx
        _YARD[key] = (dout, x, wgrad_ref(dout, x, taps, torch.float64), wgrad_ref(dout, x, taps, torch.float32), gb_serial(dout))
    return _YARD[key]


@pytest.mark.parametrize("case", c2_cases(), ids=c2_id)
def test_rounding(case):
    kernel, taps, ci, co, B, H, W, amax, sd, sx = case
    _, lib = _lib()
    dout, x, ref64, ref32, yard_b = _c2_case(case)
    dout_d, x_d = dout.to(DEV), x.to(DEV)
    k = 3 if taps == 9 else 1
    scr = int(taps == 9)
    yard_w = None
    if amax:        # the library's own wide fp32 Winograd kernel on the same inputs: the second yardstick of the conv_wh gate
        yard_w = torch.zeros(co, ci, k, k, device=DEV)
        assert _run(lib, taps, ci, co, 0, scr, 0, dout_d, x_d, yard_w, None)[0] == WINO_WIDE
        yard_w = yard_w.cpu()
    all_fails = []
    for ncu in (0, 304):
        gw = torch.zeros(co, ci, k, k, device=DEV)
        gb = torch.zeros(co, device=DEV)
        got = _run(lib, taps, ci, co, ncu, scr, amax, dout_d, x_d, gw, gb)
        assert got[0] == kernel, (KERNEL_NAMES[kernel], got)
        label = f"{c2_id(case)} ncu {ncu or _device_cus()} plan {got}"
        line, fails = noise_gate(label, gw.cpu(), gb.cpu(), ref64, ref32, kernel, K, yard_b=yard_b)
        print(line)
        all_fails += [(label, f) for f in fails]
        if amax:
            line, fails = noise_gate(label + " conv_wh gate", gw.cpu(), None, ref64, ref32, kernel, K_WH, yard_w=yard_w)
            print(line)
            all_fails += [(label + " conv_wh gate", f) for f in fails]
    assert not all_fails, all_fails
