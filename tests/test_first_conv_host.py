"""CPU: which kernel the first conv of the network takes (FwdBlock::c3_variant, csrc/fwd_plan.h) as sinddm_debug_forward_plan
reports it behind its 80 older integers, and every refusal of sinddm_debug_first_conv before a device is touched (the
pointers are made-up addresses: a call that got past its checks would fault, none may).

The rule (csrc/conv_c3m.h): conv1 of a block on the C_in = 3 route takes the matrix-core kernel in INFERENCE where
C_out % 16 == 0, C_out <= 320, the row pitch is a multiple of 4, the launch has at least 11 segments of 64 pixels per
compute unit and the rows fill their segments to 85 % or more; training, and every other shape, keeps the VALU kernel.
reference: none (which kernels an evaluation launches is this library's own business)"""
import ctypes as C

import pytest

from sinddm_amd import _lib
from test_fwd_plan_host import BLOCK0, BLOCK_INTS, N_INTS, PINNED, TINY, plan
from test_routes_host import C3, grid

N_EXT = N_INTS + 4
BADARG, BADSHAPE = -1, -2
P = 0x10000            # a 256-byte aligned address that is never dereferenced
FLOOR = 11             # SINDDM_C3M_MIN_ITEMS_PER_CU


def _ext(lib, dim_arg, train, B, H, W, ncu=256):
    out = (C.c_int64 * N_EXT)(*([-7] * N_EXT))
    assert lib.sinddm_debug_forward_plan(dim_arg, train, B, H, W, ncu, out, N_EXT) == 0
    return list(out)


def _expected(p, dim_arg, train, B, H, ncu):
    half = (dim_arg & 0xFFFF) // 2
    if p["blk"][0]["route1"] != C3:
        return 0
    takes = not train and half % 16 == 0 and half <= 320 and p["Wp"] % 4 == 0
    segs = -(-p["Wp"] // 64)
    return 2 if takes and B * H * segs >= FLOOR * ncu and p["Wp"] * 100 >= segs * 64 * 85 else 1


def test_the_older_integers_do_not_move():
    lib = _lib.load()
    for key in sorted(PINNED):
        for train in (0, 1):
            short = (C.c_int64 * N_EXT)(*([-7] * N_EXT))
            assert lib.sinddm_debug_forward_plan(key[0], train, *key[1:], 256, short, N_INTS) == 0
            full = _ext(lib, key[0], train, *key[1:])
            assert list(short)[:N_INTS] == full[:N_INTS], key
            assert list(short)[N_INTS:] == [-7] * 4, "a caller with room for 80 integers gets 80"
            assert N_INTS == BLOCK0 + 4 * BLOCK_INTS


def test_the_field_follows_the_rule_and_training_never_takes_the_new_kernel():
    lib = _lib.load()
    seen = set()
    for da, B, H, W in list(grid()) + sorted(TINY):
        for train in (0, 1):
            for ncu in (256, 64, 8):
                p = plan(lib, da, train, B, H, W, ncu)
                v = _ext(lib, da, train, B, H, W, ncu)[N_INTS:]
                assert v[0] == _expected(p, da, train, B, H, ncu), (da, train, B, H, W, ncu)
                assert v[1:] == [0, 0, 0], "only block 1 has C_in = 3"
                assert not (train and 2 in v), (da, B, H, W, ncu)
                seen.add((train, v[0]))
    assert {(0, 1), (0, 2), (1, 1)} <= seen


def test_the_benchmark_shape_and_its_neighbours():
    lib = _lib.load()
    assert _ext(lib, 160, 0, 64, 411, 512)[N_INTS] == 2             # the flagship step
    assert _ext(lib, 160, 1, 64, 411, 512)[N_INTS] == 1             # ... and its training forward
    assert _ext(lib, 160, 0, 16, 133, 177)[N_INTS] == 2             # padded rows: pitch 180 of 192, 16 x 133 x 3 = 6384 segments
    assert _ext(lib, 160, 0, 1, 20, 20)[N_INTS] == 1                # 20 segments: below the floor of 11 x 256
    assert _ext(lib, 160, 0, 16, 85, 48, 256)[N_INTS] == 1          # 1360 segments
    assert _ext(lib, 160, 0, 64, 76, 95)[N_INTS] == 1               # pitch 96 fills 75 % of its two segments
    assert _ext(lib, 160, 0, 64, 177, 220)[N_INTS] == 2             # pitch 220 of 256: 86 %
    assert _ext(lib, 10, 0, 4, 30, 30)[N_INTS] == 1                 # C_out = 5
    assert _ext(lib, 20, 0, 64, 400, 512)[N_INTS] == 1              # C_out = 10 at a large launch


def _call(lib, variant=2, ncu=256, B=2, H=9, W=36, Wt=0, co=80, x=P, w=P, bias=P, out=P, amax=None):
    return lib.sinddm_debug_first_conv(variant, ncu, B, H, W, Wt, co, x, w, bias, out, amax, None)


@pytest.mark.parametrize("kw,rc", [
    (dict(x=None), BADARG), (dict(w=None), BADARG), (dict(bias=None), BADARG), (dict(out=None), BADARG),
    (dict(variant=3), BADARG), (dict(variant=-1), BADARG),
    (dict(B=0), BADARG), (dict(H=0), BADARG), (dict(W=0), BADARG), (dict(co=0), BADARG),
    (dict(B=65536), BADSHAPE), (dict(H=1 << 14, W=1 << 14), BADSHAPE),
    (dict(Wt=32), BADSHAPE), (dict(Wt=37), BADSHAPE),         # more than three pad columns, wider than the pitch
    (dict(co=10), BADSHAPE), (dict(co=72), BADSHAPE), (dict(co=336), BADSHAPE),
    (dict(W=34), BADSHAPE), (dict(W=37), BADSHAPE),
    (dict(H=1 << 13, W=1 << 13), BADSHAPE),                   # one sample's planes beyond the 32-bit buffer
    (dict(out=P + 4), BADARG), (dict(variant=0, ncu=1, W=64, out=P + 8), BADARG),
])
def test_refusals(kw, rc):
    assert _call(_lib.load(), **kw) == rc, kw
