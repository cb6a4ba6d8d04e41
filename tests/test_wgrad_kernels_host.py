"""CPU: what tests/test_gpu_wgrad_kernels.py stands on (tests/wgrad_util.py) -- the reference, the premise that integer inputs
make every weight-gradient kernel exact, the kernels' slabs, the proof that the gates fire on an indexing defect, the case
tables against the plan at 64 / 256 / 304 compute units, and every refusal of sinddm_debug_wgrad before a device is touched.
reference SinDDM/models.py:63,65,67 (nn.Conv2d: the weight gradient is torch autograd's)"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sinddm_amd import _lib
from test_winograd_math import A2T, B2T, G2
from wgrad_util import (GRID_CASES, E_BADARG, E_BADSHAPE, GENERIC, K, NCUS, SLAB1, SLAB3, WINO, WINO_H16, WINO_WIDE, amax_allowed, c1_cases,
                        c1_inputs, c2_cases, exact_failures, exact_inputs, gb_serial, noise_gate, plan, slabs, wgrad_ref, white_inputs)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [9, 1])
def test_wgrad_ref_is_autograd_of_conv2d(taps):
    B, ci, co, H, W = 2, 5, 7, 6, 11                            # ragged everywhere
    dout, x = white_inputs((B, ci, co, H, W), 11)
    k = 3 if taps == 9 else 1
    w = torch.zeros(co, ci, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(co, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, b, padding=k // 2).backward(dout.double())
    gw, gb = wgrad_ref(dout, x, taps, torch.float64)
    assert gw.shape == w.shape and gw.dtype == torch.float64
    assert (gw - w.grad).abs().max() <= 1e-15 * w.grad.abs().max() and (gb - b.grad).abs().max() <= 1e-15 * b.grad.abs().max()


# ---- the premise of the exact cases -----------------------------------------------------------------------------------------------
def test_exact_inputs_are_small_integers():
    dout, x = exact_inputs((2, 16, 80, 5, 18), 3)
    assert set(dout.unique().tolist()) == {-1.0, 0.0, 1.0} and set(x.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert not torch.signbit(dout[dout == 0]).any() and not torch.signbit(x[x == 0]).any()


@pytest.mark.parametrize("taps", [9, 1])
def test_fp32_is_exact_on_exact_inputs(taps):
    dout, x = exact_inputs((3, 17, 33, 9, 31), 5)
    (w32, b32), (w64, b64) = wgrad_ref(dout, x, taps, torch.float32), wgrad_ref(dout, x, taps, torch.float64)
    assert torch.equal(w32.double(), w64) and torch.equal(b32.double(), b64) and w64.abs().max() > 8
    assert torch.equal(w64, w64.round())


def _f2x2_wgrad(dout, x, dtype):
    """The F(2x2,3x3) weight gradient of wgrad_wino.h in numpy `dtype`: dU = sum over 2x2 tiles of (A dY A^T) (.) (B^T d B),
    dg = G^T dU G.  Returns (dg, a bound in quarter units on every intermediate under ANY order of the sums: the transforms'
    largest value, and 4 x the largest sum over tiles of |dM V| -- a partial sum of dU cannot exceed that sum, and G^T . G, whose
    columns sum to at most 2 in magnitude, at most quadruples it, per workgroup and across the atomics of the pixel splits)."""
    A, Bt, G = (np.array(m, dtype=np.float64).astype(dtype) for m in (A2T, B2T, G2))
    A = A.T                                                     # (4, 2)
    d, xin = dout.numpy().astype(dtype), x.numpy().astype(dtype)
    B, co, H, W = d.shape
    He, We = H + H % 2, W + W % 2
    dp = np.zeros((B, co, He, We), dtype)
    dp[:, :, :H, :W] = d
    xp = np.zeros((B, xin.shape[1], He + 2, We + 2), dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = xin
    dU = np.zeros((co, xin.shape[1], 4, 4), dtype)
    absU = np.zeros(dU.shape, np.float64)
    peak = 0.0
    for ty in range(0, He, 2):
        for tx in range(0, We, 2):
            dM = np.einsum("ip,bopq,jq->boij", A, dp[:, :, ty:ty + 2, tx:tx + 2], A).astype(dtype)
            V = np.einsum("ip,bcpq,jq->bcij", Bt, xp[:, :, ty:ty + 4, tx:tx + 4], Bt).astype(dtype)
            dU += np.einsum("boij,bcij->ocij", dM, V).astype(dtype)
            absU += np.einsum("boij,bcij->ocij", np.abs(dM), np.abs(V))
            peak = max(peak, np.abs(dM).max(), np.abs(V).max())
    dg = np.einsum("ia,ocij,jb->ocab", G, dU, G).astype(dtype)
    assert dU.dtype == dtype and dg.dtype == dtype
    return dg, 4 * max(peak, 4 * absU.max())


def test_f2x2_weight_gradient_algebra_is_exact_in_fp32():
    dout, x = exact_inputs((2, 5, 6, 5, 18), 9)
    g32, peak = _f2x2_wgrad(dout, x, np.float32)
    g64, _ = _f2x2_wgrad(dout, x, np.float64)
    w64, _ = wgrad_ref(dout, x, 9, torch.float64)
    assert np.array_equal(g32.astype(np.float64), g64) and np.array_equal(g64, w64.numpy()) and 64 < peak < 2 ** 24


def test_largest_intermediate_stays_exact():
    """Bounds on the inputs, not measurements of a kernel, for the largest case of each table: direct kernels sum
    |dout in| <= 2 per pixel; a Winograd frequency sums |dM V| <= 4 x 8 per 2x2 tile and G^T . G at most quadruples it, in quarter
    units.  The sample scaled by 2^12 is beyond that crude bound, so its own sums of |dM V| are taken (_f2x2_wgrad)."""
    pix = max(c[4] * c[5] * c[6] for c in c1_cases())
    assert pix == 2 * 100 * 100 and 2 * pix < 2 ** 24
    tiles = max(c[4] * -(-c[5] // 2) * -(-c[6] // 2) for c in c1_cases() if c[0] >= WINO)
    assert 4 * (4 * 32 * tiles) < 2 ** 24
    scaled = [c for c in c1_cases() if c[9] == "scaled_sample"]
    assert scaled
    for c in scaled:                                            # ... and the reference itself is an fp32 number
        dout, x = c1_inputs(c)
        w64, b64 = wgrad_ref(dout, x, 9, torch.float64)
        g64, bound = _f2x2_wgrad(dout, x, np.float64)
        assert np.array_equal(g64, w64.numpy()) and bound < 2 ** 24, bound
        assert torch.equal(w64.float().double(), w64) and torch.equal(b64.float().double(), b64) and w64.abs().max() > 2 ** 12


# ---- slabs --------------------------------------------------------------------------------------------------------------------------
def test_slabs_tile_the_gradient_once():
    for kernel, ci, co, want in [(GENERIC, 17, 33, (3, 2)), (GENERIC, 24, 48, (3, 2)), (GENERIC, 20, 64, (2, 2)), (SLAB1, 160, 80, (1, 2)),
                                 (SLAB3, 15, 160, (2, 1)), (WINO, 160, 160, (2, 4)), (WINO_WIDE, 80, 80, (1, 2)), (WINO_H16, 40, 80, (1, 1))]:
        cover = torch.zeros(co, ci, dtype=torch.int32)
        n = 0
        for so, si in slabs(kernel, ci, co):
            cover[so, si] += 1
            n += 1
        assert (cover == 1).all() and n == want[0] * want[1], (kernel, ci, co)
    assert [s[1].stop - s[1].start for s in slabs(WINO, 160, 80)] == [48, 48, 48, 16]
    assert [s[1].stop - s[1].start for s in slabs(WINO, 80, 80)] == [48, 32] and [s[1].stop for s in slabs(WINO, 40, 80)] == [40]


# ---- the gates fire -------------------------------------------------------------------------------------------------------------------
def _mutants(dout, x, taps, dtype, kernel):
    """What three indexing defects would return, evaluated in `dtype`: one tap of the LAST slab zeroed, the last image column
    never read, one sample's contribution dropped."""
    w, b = wgrad_ref(dout, x, taps, dtype)
    so, si = list(slabs(kernel, x.shape[1], dout.shape[1]))[-1]
    tap = w.clone()
    tap[so, si, -1, 0] = 0
    d_col, x_col = dout.clone(), x.clone()
    d_col[..., -1], x_col[..., -1] = 0, 0
    return {"zero_tap_of_one_slab": (tap, b), "last_column_dropped": wgrad_ref(d_col, x_col, taps, dtype),
            "one_sample_dropped": wgrad_ref(dout[:-1], x[:-1], taps, dtype)}


@pytest.mark.parametrize("kernel,taps,ci,co", [(WINO, 9, 160, 160), (SLAB1, 1, 160, 80), (GENERIC, 9, 10, 20)])
def test_noise_gate_fires(kernel, taps, ci, co):
    dout, x = white_inputs((2, ci, co, 13, 37 if taps == 1 else 36), 21)
    ref64, ref32 = wgrad_ref(dout, x, taps, torch.float64), wgrad_ref(dout, x, taps, torch.float32)
    yard_b = gb_serial(dout)
    line, fails = noise_gate("fp32 itself", *ref32, ref64, ref32, kernel, yard_b=yard_b)
    assert not fails and "gw library" in line and "gb library" in line and "ratio 1.00" in line
    for name, (w, b) in _mutants(dout, x, taps, torch.float32, kernel).items():
        line, fails = noise_gate(name, w, b, ref64, ref32, kernel, yard_b=yard_b)
        assert fails, name
        assert ("gb" in [f[0] for f in fails]) == (name != "zero_tap_of_one_slab"), (name, fails)
        if name == "zero_tap_of_one_slab":                      # one slab in eight: only the per-slab gate names it
            so, si = list(slabs(kernel, ci, co))[-1]
            assert (so.start, so.stop, si.start, si.stop) in [f[0] for f in fails]
    # rounding alone passes: the fp32 reference with its last bit flipped on every element is inside K
    flipped = (ref32[0].view(torch.int32) ^ 1).view(torch.float32)
    assert not noise_gate("ulp", flipped, ref32[1], ref64, ref32, kernel, k=K, yard_b=yard_b)[1]
    assert not noise_gate("serial gb", ref32[0], yard_b, ref64, ref32, kernel, yard_b=yard_b)[1]
    # gb: one image row lost fails, and so does rounding alone once it is worse than fp32's: row sums kept in binary16
    lost = ref32[1] - wgrad_ref(dout[:, :, :1], x[:, :, :1], taps, torch.float32)[1]
    assert [f[0] for f in noise_gate("lost row", ref32[0], lost, ref64, ref32, kernel, yard_b=yard_b)[1]] == ["gb"]
    half = dout.double().sum(3).half().double().sum((0, 2)).float()
    assert [f[0] for f in noise_gate("binary16 partial sums", ref32[0], half, ref64, ref32, kernel, yard_b=yard_b)[1]] == ["gb"]


def test_gb_serial_is_one_accumulator_per_channel():
    dout, _ = white_inputs((2, 3, 7, 13, 37), 31)
    v = dout.permute(1, 0, 2, 3).reshape(7, -1).numpy()
    acc = np.zeros(7, np.float32)
    for i in range(v.shape[1]):
        acc = acc + v[:, i]
    assert acc.dtype == np.float32 and np.array_equal(gb_serial(dout).numpy(), acc)
    # n - 1 = 961 adds of half an ulp each at the most (Higham 4.2: gamma_(n-1) sum |dout|, gamma_n = n u / (1 - n u), u = 2^-24)
    bound = 961 * 2.0 ** -24 / (1 - 961 * 2.0 ** -24) * dout.double().abs().sum((0, 2, 3))
    assert ((gb_serial(dout).double() - dout.double().sum((0, 2, 3))).abs() <= bound).all()


@pytest.mark.parametrize("kernel,taps,ci,co", [(WINO_WIDE, 9, 160, 80), (SLAB3, 9, 15, 80), (GENERIC, 1, 80, 3)])
def test_exact_gate_fires(kernel, taps, ci, co):
    dout, x = exact_inputs((2, ci, co, 5, 20), 23)
    w64, b64 = wgrad_ref(dout, x, taps, torch.float64)
    assert exact_failures(w64.float(), b64.float(), w64, b64, kernel) == []
    assert exact_failures(2 * w64.float(), 2 * b64.float(), w64, b64, kernel, times=2) == []
    assert exact_failures(w64.float(), b64.float(), w64, b64, kernel, times=2)
    for name, (w, b) in _mutants(dout, x, taps, torch.float32, kernel).items():
        fails = exact_failures(w, b, w64, b64, kernel)
        assert fails, name
        if name == "zero_tap_of_one_slab":
            so, si = list(slabs(kernel, ci, co))[-1]
            assert [f[0] for f in fails] == [(so.start, so.stop, si.start, si.stop)]
    one = w64.float().clone()
    one[-1, -1, 0, 0] += 1                                      # a single element off by one unit
    assert len(exact_failures(one, b64.float(), w64, b64, kernel)) == 1
    assert exact_failures(w64.float(), b64.float() + 1, w64, b64, kernel)[0][0] == "gb"


# ---- the tables against the plan -----------------------------------------------------------------------------------------------------
def test_c1_table_reaches_the_kernel_it_names_on_every_grid():
    lib = _lib.load()
    cases = c1_cases()
    assert len(cases) == len(set(cases))
    for c in cases:
        kernel, taps, ci, co, B, H, W, scr, amax, variant = c
        for ncu in NCUS:
            assert plan(lib, taps, ci, co, B, H, W, scr, amax, ncu)[0] == kernel, (c, ncu)
        if kernel == WINO_H16:
            assert amax_allowed(ci, co) and W % 4 == 0
    # the edges the table is there for
    assert any(c[0] == SLAB3 and not c[7] for c in cases) and any(c[0] == SLAB3 and c[2] == 1024 for c in cases)
    assert {c[2] for c in cases if c[0] in (WINO, WINO_WIDE)} >= {16, 40, 80, 160}
    assert plan(lib, 9, 15, 80, 1, 9, 33, 1, 0, 256)[0] == SLAB3 and plan(lib, 9, 16, 80, 1, 9, 33, 1, 0, 256)[0] == WINO
    # fewer pixel tiles than splits, and grids that differ between the three device sizes
    assert plan(lib, 9, 10, 20, 1, 2, 5, 0, 0, 256)[2] == 8 and plan(lib, 1, 40, 80, 1, 1, 1, 0, 0, 256)[2] == 8
    assert len({plan(lib, 9, 160, 160, 1, 13, 64, 1, 0, n) for n in NCUS}) >= 2
    # ... and the cases that are there for the grids: three device sizes, three grids
    for kernel, taps, ci, co, B, H, W, scr, amax, variant in GRID_CASES:
        assert len({plan(lib, taps, ci, co, B, H, W, scr, amax, n) for n in NCUS}) == 3, (kernel, ci, co, B, H, W)
    assert {c[0] for c in GRID_CASES} == {SLAB1, SLAB3, WINO, WINO_WIDE, WINO_H16}


def test_c2_table_reaches_the_kernel_it_names_and_every_kernel():
    lib = _lib.load()
    cases = c2_cases()
    assert len(cases) == len(set(cases))
    for c in cases:
        kernel, taps, ci, co, B, H, W, amax, sd, sx = c
        for ncu in NCUS:
            assert plan(lib, taps, ci, co, B, H, W, int(taps == 9), amax, ncu)[0] == kernel, (c, ncu)
        assert (kernel == WINO_H16) == bool(amax)
    assert {c[0] for c in cases} == set(range(GENERIC, WINO_H16 + 1))


# ---- the hook's refusals (before any device call) --------------------------------------------------------------------------------------
def _call(lib, taps=9, ci=160, co=160, B=2, H=5, W=20, ncu=256, scr=1, amax=0, dout=0x10000, x=0x20000, gw=0x30000, gb=0x40000,
          scratch=0x100000, nbytes=None, out=True):
    plan_out = (C.c_int * 4)(-7, -7, -7, -7)
    if nbytes is None:
        nbytes = lib.sinddm_debug_wgrad_scratch_bytes(taps, ci, co, B)
    rc = lib.sinddm_debug_wgrad(taps, ci, co, B, H, W, ncu, scr, amax, dout, x, gw, gb, scratch, nbytes, plan_out if out else None, None)
    return rc, list(plan_out)


def test_hook_refuses_before_any_device_call():
    """Every pointer here is a made-up address: a refusal that came after a device call would fault, not return."""
    lib = _lib.load()
    for kw in (dict(dout=None), dict(x=None), dict(gw=None), dict(scratch=None), dict(out=False)):
        assert _call(lib, **kw)[0] == E_BADARG, kw
    for kw in (dict(ci=0), dict(co=0), dict(B=0), dict(H=0), dict(W=-1), dict(taps=3), dict(taps=0), dict(taps=25)):
        assert _call(lib, nbytes=1 << 30, **kw)[0] == E_BADARG, kw
    full = lib.sinddm_debug_wgrad_scratch_bytes(9, 160, 160, 2)
    assert full == 256 + 160 * 160 * 9 * 4 + 2 * 256
    assert lib.sinddm_debug_wgrad_scratch_bytes(1, 160, 80, 3) == 256 + 2 * 256
    assert lib.sinddm_debug_wgrad_scratch_bytes(3, 160, 80, 3) == 0 == lib.sinddm_debug_wgrad_scratch_bytes(9, 0, 80, 3)
    # scratch: the zero page alone, + the slab, + the maxima
    assert _call(lib, scr=0, nbytes=255)[0] == E_BADARG
    assert _call(lib, scr=1, nbytes=full - 2 * 256 - 1)[0] == E_BADARG
    assert _call(lib, scr=1, amax=1, nbytes=full - 1)[0] == E_BADARG
    assert _call(lib, scratch=0x100010)[0] == E_BADARG
    # alignment: 16 bytes where the plan takes a wide kernel, 4 everywhere
    assert _call(lib, dout=0x10004)[0] == E_BADARG and _call(lib, x=0x20008)[0] == E_BADARG
    assert _call(lib, dout=0x10002, W=18)[0] == E_BADARG and _call(lib, gw=0x30002)[0] == E_BADARG and _call(lib, gb=0x40001)[0] == E_BADARG
    # use_amax where production has no maxima
    assert _call(lib, taps=1, amax=1)[0] == E_BADARG and _call(lib, scr=0, amax=1)[0] == E_BADARG
    for kw in (dict(W=18), dict(ci=16, co=80), dict(ci=40, co=80), dict(ci=160, co=48), dict(ci=3, co=80)):
        assert _call(lib, amax=1, **kw)[0] == E_BADSHAPE, kw
    assert _call(lib, amax=1, B=65536)[0] == E_BADSHAPE        # the maxima kernel's gridDim.y
    # sizes beyond the kernels' 32-bit indexing
    assert _call(lib, ci=3, co=3, B=1, H=1 << 14, W=1 << 16, scr=0)[0] == E_BADSHAPE
    assert _call(lib, ci=3, co=80, B=1, H=1 << 12, W=1 << 10, scr=0)[0] == E_BADSHAPE
    assert _call(lib, ci=1 << 14, co=1 << 14, nbytes=1 << 40)[0] == E_BADSHAPE
    # nothing was reported for a refused call
    assert _call(lib, dout=0x10004)[1] == [-7] * 4
