"""CPU: ForwardPlan::head_proj (csrc/fwd_plan.h) as sinddm_debug_forward_plan reports it behind its older integers.

head_proj = block 3's second conv (conv_wr_kernel) forms the head's projection W_r x_in of its own output in its epilogue
and the collapsed head reads those 3 planes instead of the dim planes of block 4's input.  It must hold exactly where
  * the evaluation runs the collapsed head (inference),
  * block 3's conv2 is on conv_wh with items of 160 output channels,
  * and that is every channel of the tensor: dim = 160 (240 is no multiple of 160; at 320 an item holds half a pixel's channels),
and nowhere under SINDDM_DIM_HEAD_XIN, SINDDM_DIM_FP32_CONVS or in training.  The launch count and every older integer are
the same with and without it: the projection costs no launch and no workspace.
Over every scale of the C2 and C3 pyramids at their batch sizes, dim 80 / 160 / 240 / 320, 64 / 256 / 304 compute units.
reference: none (which kernels an evaluation launches is this library's own business)"""
import ctypes as C
import os
import re

import pytest

from sinddm_amd import _lib
from sinddm_amd.configs import CONFIGS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_INTS, N_EXT, N_EXT2 = 80, 84, 85
BLOCK0, BLOCK_INTS = 24, 14
WH = 8
FP32, XIN = _lib.DIM_FP32_CONVS, _lib.DIM_HEAD_XIN
SHAPES = [(CONFIGS[c]["batch"], h, w) for c in ("C2", "C3") for (w, h) in CONFIGS[c]["sizes"]]
DIMS = (80, 160, 240, 320)


def _plan(lib, dim_arg, train, B, H, W, ncu, cap=N_EXT2):
    out = (C.c_int64 * N_EXT2)(*([-7] * N_EXT2))
    assert lib.sinddm_debug_forward_plan(dim_arg, train, B, H, W, ncu, out, cap) == 0
    return list(out)


def test_option_bit_and_header_agree():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    assert int(re.search(r"#define SINDDM_DIM_HEAD_XIN (0x[0-9a-fA-F]+)", txt).group(1), 16) == XIN == 0x20000
    dbg = open(os.path.join(REPO, "include", "sinddm_hip_debug.h")).read()
    assert "#define SINDDM_FWD_PLAN_INTS_EXT2 (SINDDM_FWD_PLAN_INTS_EXT + 1)" in dbg
    lib = _lib.load()
    # the option changes no layout; the bit above it is still no network
    assert lib.sinddm_param_count(160 | XIN) == lib.sinddm_param_count(160)
    assert lib.sinddm_packed_count(160 | XIN) == lib.sinddm_packed_count(160)
    assert lib.sinddm_workspace_bytes(160 | XIN, 16, 186, 248) == lib.sinddm_workspace_bytes(160, 16, 186, 248)
    assert lib.sinddm_param_count(160 | 0x40000) == -1
    from sinddm_amd.models import SinDDMNet
    assert SinDDMNet.head_xin is False


@pytest.mark.parametrize("dim", DIMS)
def test_head_proj_follows_its_rule(dim):
    lib = _lib.load()
    seen = set()
    for B, H, W in SHAPES:
        for ncu in (256, 64, 304):
            where = (dim, B, H, W, ncu)
            p = _plan(lib, dim, 0, B, H, W, ncu)
            blk3 = p[BLOCK0 + 2 * BLOCK_INTS:BLOCK0 + 3 * BLOCK_INTS]
            head, route2, variant2 = p[4], blk3[1], blk3[3]
            want = int(bool(head) and route2 == WH and variant2 == 2 and dim == 160)
            assert p[N_EXT] == want, where
            seen.add(want)
            # the older integers do not move and do not change: a caller with less room gets the same ones, untouched behind
            for cap in (N_INTS, N_EXT):
                q = _plan(lib, dim, 0, B, H, W, ncu, cap)
                assert q[:cap] == p[:cap] and q[cap:] == [-7] * (N_EXT2 - cap), where
            # the x_in option: the same plan (launch count, workspace, routes) without the flag
            x = _plan(lib, dim | XIN, 0, B, H, W, ncu)
            assert x[:N_EXT] == p[:N_EXT] and x[N_EXT] == 0, where
            # fp32 convs never route conv_wh; training keeps block 4's output
            assert _plan(lib, dim | FP32, 0, B, H, W, ncu)[N_EXT] == 0, where
            assert _plan(lib, dim, 1, B, H, W, ncu)[N_EXT] == 0, where
    assert seen == ({0, 1} if dim == 160 else {0}), (dim, seen)


def test_headline_and_smallest_routed_shapes():
    lib = _lib.load()
    # C3's finest scale at batch 64 (the benchmark's headline) and the smallest C2 shape the plan hands to conv_wr_kernel
    # on 256 compute units; one scale below it the launch keeps the 80-channel kernel
    assert _plan(lib, 160, 0, 64, 411, 512, 256)[N_EXT] == 1
    assert _plan(lib, 160, 0, 16, 186, 248, 256)[N_EXT] == 1
    assert _plan(lib, 160, 0, 16, 133, 177, 256)[N_EXT] == 0
    assert _plan(lib, 320, 0, 64, 411, 512, 256)[N_EXT] == 0
