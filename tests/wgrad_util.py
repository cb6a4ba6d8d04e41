"""Shared by tests/test_wgrad_kernels_host.py and tests/test_gpu_wgrad_kernels.py (CPU only, no device call here): the plain
reference of ONE weight-gradient launch, inputs on which every kernel must be exact, the kernels' own slabs, the gates, and
the tables of cases.

Why exact inputs: a weight gradient is a sum over every pixel of the batch, and rel-L2 with a tolerance cannot tell an
indexing defect in one tile from the rounding of that sum.  With dout in {-1, 0, 1} and in in {-2 .. 2}
  * every product and every partial sum of the direct kernels is an integer far below 2^24: fp32 adds them exactly in any order;
  * the F(2x2) transforms A dY A^T and B^T d B are +-1 sums (integers), the frequency sums dU are integers, and G^T dU G
    (G carries 0.5) produces only multiples of 1/4: exact while 4 |value| < 2^24;
  * the binary16 kernel scales by a power of two taken from the operands' maxima: |dM| <= 4 and |V| <= 8 times that power are
    binary16 numbers, so the low piece of the hi/lo split is zero and the matrix pipe multiplies exact integers;
so each of the six kernels must return the float64 reference BIT FOR BIT, whatever the order of its atomics, its pixel
splits or its launch table.
reference SinDDM/models.py:63,65,67 (nn.Conv2d; the gradient is torch autograd's)"""
import ctypes as C

import torch
import torch.nn.functional as F

from conftest import rel_l2
from sinddm_amd.synth import hash_randn

GENERIC, SLAB1, SLAB3, WINO, WINO_WIDE, WINO_H16 = range(6)
KERNEL_NAMES = ("generic", "slab1x1", "slab3x3", "wino_dword", "wino_wide", "wino_binary16")
NCUS = (64, 256, 304)
K = 3            # tests/test_gpu_fullrank.py: the factor over the fp32 evaluation's own error (doubled for sub-regions)
K_WH = 1.5       # conv_wh's gate (tests/test_gpu_h2.py, test_gpu_fullrank.py): over max(fp32 yardstick, the library's fp32 kernel)
E_BADARG, E_BADSHAPE = -1, -2


# ---- the reference -------------------------------------------------------------------------------------------------------------
def wgrad_ref(dout, x, taps, dtype):
    """gw (C_out, C_in, k, k), k = 3 or 1:  gw[co,ci,ky,kx] = sum_{b,y,x} dout[b,co,y,x] x_pad[b,ci,y+ky-1,x+kx-1];  gb = sum dout."""
    d, xin = dout.to(dtype), x.to(dtype)
    H, W = d.shape[2:]
    gb = d.sum((0, 2, 3))
    if taps == 1:
        return torch.einsum("bohw,bihw->oi", d, xin)[:, :, None, None].contiguous(), gb
    assert taps == 9
    xp = F.pad(xin, (1, 1, 1, 1))
    rows = [torch.stack([torch.einsum("bohw,bihw->oi", d, xp[:, :, ky:ky + H, kx:kx + W]) for kx in range(3)], -1) for ky in range(3)]
    return torch.stack(rows, -2).contiguous(), gb


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def exact_inputs(shape, key):
    """shape = (B, C_in, C_out, H, W) -> integer-valued fp32 (dout in {-1, 0, 1}, in in {-2 .. 2}), all values present."""
    B, cin, cout, H, W = shape
    dout = (hash_randn((B, cout, H, W), key) * 0.9).round().clamp(-1, 1)
    x = (hash_randn((B, cin, H, W), key + 1) * 1.3).round().clamp(-2, 2)
    return dout + 0.0, x + 0.0          # (+ 0.0: no negative zeros)


def white_inputs(shape, key):
    """White operands as training hands them over: dout scaled by 1 / (B 3 H W), the gradient of an L1-mean loss."""
    B, cin, cout, H, W = shape
    return hash_randn((B, cout, H, W), key) / (B * 3 * H * W), hash_randn((B, cin, H, W), key + 1)


# ---- slabs -----------------------------------------------------------------------------------------------------------------------
def mt_for(cout):
    return 5 if cout % 80 == 0 else 2 if cout % 32 == 0 else 1


def slabs(kernel, cin, cout):
    """The (co slice, ci slice) blocks of the gradient one workgroup of `kernel` owns: 16 mt x 16 (generic), 80 x 80 (slab
    kernels), 80 x 48 (Winograd domain).  The last block of an axis may be ragged."""
    co, ci = {GENERIC: (16 * mt_for(cout), 16), SLAB1: (80, 80), SLAB3: (80, 80)}.get(kernel, (80, 48))
    for o in range(0, cout, co):
        for i in range(0, cin, ci):
            yield slice(o, min(o + co, cout)), slice(i, min(i + ci, cin))


# ---- gates -----------------------------------------------------------------------------------------------------------------------
def exact_failures(got_w, got_b, ref_w, ref_b, kernel, times=1):
    """[] iff got == times * float64 reference, bit for bit (references are cast to fp32: they are integers).  Otherwise the
    slabs that differ, with the number of wrong elements and the first wrong index -- what localises a defect."""
    want_w, want_b = (ref_w * times).float(), (ref_b * times).float()
    fails = []
    if got_b is not None and not torch.equal(got_b, want_b):
        fails.append(("gb", int((got_b != want_b).sum()), (got_b != want_b).nonzero()[0].tolist()))
    if not torch.equal(got_w, want_w):
        for so, si in slabs(kernel, ref_w.shape[1], ref_w.shape[0]):
            bad = got_w[so, si] != want_w[so, si]
            if bad.any():
                fails.append(((so.start, so.stop, si.start, si.stop), int(bad.sum()), bad.nonzero()[0].tolist()))
        assert fails                    # (NaNs and shape mismatches cannot hide: torch.equal said no)
    return fails


def gb_serial(dout):
    """gb in fp32 as a plain loop adds it: one accumulator per channel over the pixels in (b, y, x) order.  The second fp32
    evaluation of the bias gradient's yardstick (noise_gate)."""
    v = dout.float().permute(1, 0, 2, 3).reshape(dout.shape[1], -1)
    acc = torch.zeros(dout.shape[1], dtype=torch.float32)
    for i in range(v.shape[1]):
        acc = acc + v[:, i]
    return acc


def noise_gate(label, got_w, got_b, ref64, ref32, kernel, k=K, yard_w=None, yard_b=None):
    """rel-L2 against float64 <= k x the rel-L2 of an fp32 evaluation on the CPU, per tensor, and for gw per slab with the
    factor doubled.
    gw: the fp32 evaluation is wgrad_ref(float32).  `yard_w` (the library's fp32 Winograd kernel on the same inputs) widens the
    yardstick to the larger of the two fp32 errors, as the conv_wh gate does.
    gb (judged when `yard_b` = gb_serial(dout) is given): the yardstick is the larger error of two fp32 evaluations, torch's sum
    and the serial loop.  torch sums pairwise, to within half an ulp of the result, which no kernel that meets its pixel splits
    with atomics can be held to a multiple of: the kernels add short serial chains per lane, a shuffle tree, and then one
    atomic per split in an order that changes from launch to launch.  A serial fp32 sum is the plain evaluation of the same
    kind, with chains at least as long as any kernel's.
    Returns (the printed line, failures)."""
    (w64, b64), (w32, b32) = ref64, ref32
    assert torch.isfinite(got_w).all() and (got_b is None or torch.isfinite(got_b).all()), label
    fails, parts = [], []
    e_k, e_32 = rel_l2(got_w, w64), rel_l2(w32, w64)
    e_y = max(e_32, rel_l2(yard_w, w64) if yard_w is not None else 0.0)
    parts.append(f"gw library {e_k:.3e} fp32 {e_y:.3e} ratio {e_k / max(e_y, 1e-30):.2f}")
    if not e_k <= k * e_y:
        fails.append(("gw", e_k, e_y))
    if yard_b is not None:
        e_k, e_y = rel_l2(got_b, b64), max(rel_l2(b32, b64), rel_l2(yard_b, b64))
        parts.append(f"gb library {e_k:.3e} fp32 {e_y:.3e} ratio {e_k / max(e_y, 1e-30):.2f}")
        if not e_k <= k * e_y:
            fails.append(("gb", e_k, e_y))
    worst = (0.0, None)
    for so, si in slabs(kernel, w64.shape[1], w64.shape[0]):
        e_k, e_32 = rel_l2(got_w[so, si], w64[so, si]), rel_l2(w32[so, si], w64[so, si])
        e_y = max(e_32, rel_l2(yard_w[so, si], w64[so, si]) if yard_w is not None else 0.0)
        ratio = e_k / max(e_y, 1e-30)
        if ratio > worst[0]:
            worst = (ratio, (so.start, so.stop, si.start, si.stop))
        if not e_k <= 2 * k * e_y:
            fails.append(((so.start, so.stop, si.start, si.stop), e_k, e_y))
    line = f"[{label}] vs float64 rel-L2: " + "; ".join(parts) + f"; worst slab {worst[1]} ratio {worst[0]:.2f} (allowed {k}, slab {2 * k})"
    return line, fails


# ---- the cases -------------------------------------------------------------------------------------------------------------------
GEN_SHAPES = [(1, 1, 1), (1, 2, 5), (2, 3, 33), (1, 5, 64), (3, 9, 31)]
SLAB1_HW = [(1, 1), (7, 9), (8, 8), (5, 13), (3, 43)]                     # H W = 1, 63, 64, 65, 129
WINO_SHAPES = [(1, 1, 1), (1, 3, 5), (3, 4, 17), (2, 5, 18), (1, 9, 33)]
WIDE_SHAPES = [(1, 1, 4), (1, 4, 16), (2, 5, 20), (1, 9, 36), (1, 13, 64)]
WINO_CH = [(16, 80), (40, 80), (80, 160), (160, 160), (160, 80)]


def amax_allowed(cin, cout):
    """The channel part of sinddm_debug_wgrad's use_amax rule (include/sinddm_hip_debug.h)."""
    return cin % 80 == 0 and cout % 80 == 0


def c1_cases():
    """(kernel, taps, C_in, C_out, B, H, W, have_scr, use_amax, variant) of the exact cases; variant: None, 'zero_sample' or
    'scaled_sample' (binary16 only)."""
    out = []
    for taps in (9, 1):
        chans = [(3, 10), (10, 20), (20, 20), (17, 33), (24, 48)] + ([(10, 3), (80, 3)] if taps == 1 else [])
        out += [(GENERIC, taps, ci, co, *s, 0, 0, None) for ci, co in chans for s in GEN_SHAPES]
    out += [(SLAB1, 1, ci, co, B, h, w, 0, 0, None) for ci, co in [(3, 80), (40, 80), (80, 160), (160, 80)] for h, w in SLAB1_HW
            for B in (1, 3)]
    out += [(SLAB3, 9, ci, co, *s, scr, 0, None) for ci, co in [(3, 80), (15, 80), (8, 160)] for s in GEN_SHAPES for scr in (1, 0)]
    out.append((SLAB3, 9, 1024, 1040, 1, 2, 3, 1, 0, None))               # 13 x 22 = 286 slabs do not fit the launch table
    out += [(WINO, 9, ci, co, *s, 1, 0, None) for ci, co in WINO_CH for s in WINO_SHAPES]
    out += [(WINO_WIDE, 9, ci, co, *s, 1, 0, None) for ci, co in WINO_CH for s in WIDE_SHAPES]
    for ci, co in [c for c in WINO_CH if amax_allowed(*c)]:
        out += [(WINO_H16, 9, ci, co, *s, 1, 1, None) for s in WIDE_SHAPES]
    out += [(WINO_H16, 9, 160, 160, 2, 5, 20, 1, 1, v) for v in ("zero_sample", "scaled_sample")]
    return out + GRID_CASES


# The shapes above are so small that the number of pixel tiles caps every grid: 64, 256 and 304 compute units launch the
# same workgroups there.  These have enough tiles for three different grids per case (asserted on the host), still a few
# thousand pixels: the slab kernels need >= 304 tiles per slab, the Winograd launch table >= its largest per-slab share.
# (The generic kernel's split budget is a constant: its grid never depends on the device.)
GRID_CASES = [(SLAB1, 1, 40, 80, 2, 100, 100, 0, 0, None),                # 2 x 157 flat 64-pixel tiles
              (SLAB3, 9, 3, 80, 2, 20, 500, 1, 0, None),                  # 2 x 10 x 16 tiles of 2 x 32
              (WINO, 9, 160, 160, 2, 20, 67, 1, 0, None),                 # 2 x 5 x 5 tiles of 4 x 16, 8 slabs
              (WINO_WIDE, 9, 160, 160, 2, 20, 68, 1, 0, None),
              (WINO_H16, 9, 160, 160, 2, 20, 68, 1, 1, None),
              (WINO, 9, 80, 160, 2, 28, 99, 1, 0, None),                  # 2 x 7 x 7 tiles, 4 slabs (48 + 32)
              (WINO_WIDE, 9, 80, 160, 2, 28, 100, 1, 0, None),
              (WINO_H16, 9, 80, 160, 2, 28, 100, 1, 1, None)]


def case_id(c):
    kernel, taps, ci, co, B, H, W, scr, amax, variant = c
    return f"{KERNEL_NAMES[kernel]}_t{taps}_{ci}to{co}_{B}x{H}x{W}" + ("" if scr or kernel != SLAB3 else "_noscr") + (f"_{variant}" if variant else "")


def c1_inputs(c):
    kernel, taps, ci, co, B, H, W, scr, amax, variant = c
    dout, x = exact_inputs((B, ci, co, H, W), 7000 + 131 * ci + 17 * co + 5 * W + H + taps)
    if variant == "zero_sample":
        dout[1], x[1] = 0.0, 0.0             # its maximum is 0: the launch's scale comes from the other sample
    elif variant == "scaled_sample":
        dout[1] *= 2.0 ** 12                 # the launch's scale follows it: sample 0 sits 12 bits lower in the binary16 range, still exact
    return dout, x


# C2: (kernel, taps, C_in, C_out, B, H, W, use_amax, scale of dout, scale of in)
def c2_cases():
    out = []
    for s in [(2, 13, 36), (3, 9, 33)]:
        out += [(GENERIC, 9, 10, 20, *s, 0, 1.0, 1.0), (SLAB3, 9, 3, 80, *s, 0, 1.0, 1.0)]
    for ci, co in [(80, 160), (160, 160), (160, 80)]:
        out += [(WINO_WIDE, 9, ci, co, 2, 13, 36, 0, 1.0, 1.0), (WINO_H16, 9, ci, co, 2, 13, 36, 1, 1.0, 1.0),
                (WINO, 9, ci, co, 3, 9, 33, 0, 1.0, 1.0)]
    out.append((WINO_H16, 9, 160, 160, 2, 13, 36, 1, 2.0 ** -12, 2.0 ** 10))
    out += [(GENERIC, 1, ci, co, 2, 13, 37, 0, 1.0, 1.0) for ci, co in [(10, 20), (80, 3)]]
    out += [(SLAB1, 1, ci, co, 2, 13, 37, 0, 1.0, 1.0) for ci, co in [(3, 80), (80, 160), (160, 160), (160, 80)]]
    return out


def c2_id(c):
    kernel, taps, ci, co, B, H, W, amax, sd, sx = c
    return f"{KERNEL_NAMES[kernel]}_t{taps}_{ci}to{co}_{B}x{H}x{W}" + ("_scaled" if sd != 1.0 else "")


# ---- the plan, on the host ---------------------------------------------------------------------------------------------------------
def plan(lib, taps, ci, co, B, H, W, scr, amax, ncu):
    """(kernel, workgroups, S, staged) of sinddm_debug_wgrad_plan on `ncu` > 0 compute units, and for the Winograd kernels the
    launch table behind it: two counts with the same answer launch the same grid."""
    assert ncu > 0
    out = (C.c_int * 4)()
    assert lib.sinddm_debug_wgrad_plan(taps, ci, co, B, H, W, scr, amax, ncu, out) == 0
    key = tuple(out)
    if out[0] >= WINO:
        wg, sp = (C.c_uint32 * 512)(), (C.c_int32 * 256)()
        n = lib.sinddm_debug_wgrad_map(ci, co, B * -(-W // 16) * -(-H // 4), ncu, wg, 512, sp, 256)
        assert n == out[1]
        key += (tuple(wg[:n]),)
    return key
