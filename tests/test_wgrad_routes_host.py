"""CPU: which kernel and grid every weight-gradient launch of sinddm_net_backward takes (wgrad_plan, wgrad_plan.h) as
sinddm_debug_wgrad_routes reports it: 17 launches x (kernel, workgroups, S, staged), in launch order.

The pinned rows were taken at 256 compute units from the commit before the weight gradients had a plan (its launcher patched
to return its decision in front of its first device call); the whole grid of test_routes_host.py agreed at 256, 64 and 304
compute units (3888 rows).
reference: none (which kernel runs is this library's own business; the numbers are gated in test_gpu_train.py)
"""
import ctypes as C
import inspect

import pytest

from sinddm_amd import _lib
from test_routes_host import FP32, WH, grid

GENERIC, SLAB1, SLAB3, WINO, WINO_WIDE, WINO_H16, DW_TILES, DW_ROWS = range(8)
NCUS = (256, 64, 304)

# (dim_arg, B, H, W) -> the 17 launches at 256 CUs: final 1x1, then block 3..0: conv2, residual 1x1, conv1, depthwise
PINNED = {
    (160, 64, 411, 512): [0, 1000, 200, 0, 5, 256, 0, 1, 1, 256, 128, 0, 5, 256, 0, 1, 7, 10240, 0, 0, 5, 256, 0, 1, -1, -1, -1, -1, 5, 256, 0, 1, 7, 10240, 0, 0, 5, 256, 0, 1, 1, 256, 128, 0, 5, 256, 0, 1, 7, 5120, 0, 0, 5, 256, 0, 1, 1, 256, 256, 0, 2, 256, 256, 1, 7, 192, 0, 0],
    (160 | FP32, 64, 411, 512): [0, 1000, 200, 0, 4, 256, 0, 1, 1, 256, 128, 0, 4, 256, 0, 1, 7, 10240, 0, 0, 4, 256, 0, 1, -1, -1, -1, -1, 4, 256, 0, 1, 7, 10240, 0, 0, 4, 256, 0, 1, 1, 256, 128, 0, 4, 256, 0, 1, 7, 5120, 0, 0, 4, 256, 0, 1, 1, 256, 256, 0, 2, 256, 256, 1, 7, 192, 0, 0],
    (160, 16, 133, 177): [0, 1000, 200, 0, 3, 256, 0, 1, 1, 256, 128, 0, 3, 256, 0, 1, 6, 2560, 0, 0, 3, 256, 0, 1, -1, -1, -1, -1, 3, 256, 0, 1, 6, 2560, 0, 0, 3, 256, 0, 1, 1, 256, 128, 0, 3, 256, 0, 1, 6, 1280, 0, 0, 3, 256, 0, 1, 1, 256, 256, 0, 2, 256, 256, 1, 6, 48, 0, 0],
    (160, 1, 20, 20): [0, 80, 16, 0, 4, 20, 0, 1, 1, 16, 8, 0, 4, 40, 0, 1, 6, 160, 0, 0, 4, 80, 0, 1, -1, -1, -1, -1, 4, 80, 0, 1, 6, 160, 0, 0, 4, 80, 0, 1, 1, 16, 8, 0, 4, 40, 0, 1, 6, 80, 0, 0, 4, 20, 0, 1, 1, 8, 8, 0, 2, 16, 16, 1, 6, 3, 0, 0],
    (160, 2, 9, 11): [0, 80, 16, 0, 3, 12, 0, 1, 1, 16, 8, 0, 3, 24, 0, 1, 6, 320, 0, 0, 3, 48, 0, 1, -1, -1, -1, -1, 3, 48, 0, 1, 6, 320, 0, 0, 3, 48, 0, 1, 1, 16, 8, 0, 3, 24, 0, 1, 6, 160, 0, 0, 3, 12, 0, 1, 1, 8, 8, 0, 2, 16, 16, 1, 6, 6, 0, 0],
    (80, 16, 186, 248): [0, 1008, 336, 0, 0, 1008, 112, 0, 0, 960, 64, 0, 0, 960, 64, 0, 7, 1280, 0, 0, 5, 256, 0, 1, -1, -1, -1, -1, 5, 256, 0, 1, 7, 1280, 0, 0, 5, 256, 0, 1, 1, 256, 256, 0, 4, 256, 0, 1, 7, 640, 0, 0, 0, 1008, 112, 0, 0, 1008, 336, 0, 0, 1008, 336, 0, 7, 48, 0, 0],
    (80, 4, 411, 512): [0, 1008, 336, 0, 0, 1008, 112, 0, 0, 960, 64, 0, 0, 960, 64, 0, 7, 320, 0, 0, 5, 256, 0, 1, -1, -1, -1, -1, 5, 256, 0, 1, 7, 320, 0, 0, 5, 256, 0, 1, 1, 256, 256, 0, 4, 256, 0, 1, 7, 160, 0, 0, 0, 1008, 112, 0, 0, 1008, 336, 0, 0, 1008, 336, 0, 7, 12, 0, 0],
    (20, 4, 133, 177): [0, 1024, 1024, 0, 0, 1024, 1024, 0, 0, 1024, 512, 0, 0, 1024, 512, 0, 6, 80, 0, 0, 0, 1024, 256, 0, -1, -1, -1, -1, 0, 1024, 256, 0, 6, 80, 0, 0, 0, 1024, 256, 0, 0, 1024, 512, 0, 0, 1024, 512, 0, 6, 40, 0, 0, 0, 1024, 1024, 0, 0, 1024, 1024, 0, 0, 1024, 1024, 0, 6, 12, 0, 0],
    (10, 4, 30, 30): [0, 64, 64, 0, 0, 64, 64, 0, 0, 64, 64, 0, 0, 64, 64, 0, 6, 40, 0, 0, 0, 64, 64, 0, -1, -1, -1, -1, 0, 64, 64, 0, 6, 40, 0, 0, 0, 64, 64, 0, 0, 64, 64, 0, 0, 64, 64, 0, 6, 20, 0, 0, 0, 64, 64, 0, 0, 64, 64, 0, 0, 64, 64, 0, 6, 12, 0, 0],
    (240, 32, 96, 128): [0, 1024, 128, 0, 0, 1024, 16, 0, 0, 960, 8, 0, 0, 960, 8, 0, 6, 7680, 0, 0, 5, 256, 0, 1, -1, -1, -1, -1, 5, 256, 0, 1, 6, 7680, 0, 0, 5, 256, 0, 1, 1, 240, 40, 0, 4, 256, 0, 1, 6, 3840, 0, 0, 0, 1024, 16, 0, 0, 1024, 128, 0, 0, 1024, 128, 0, 6, 96, 0, 0],
    (48, 1, 67, 90): [0, 208, 104, 0, 0, 416, 104, 0, 0, 624, 104, 0, 0, 624, 104, 0, 6, 48, 0, 0, 0, 936, 104, 0, -1, -1, -1, -1, 0, 936, 104, 0, 6, 48, 0, 0, 0, 936, 104, 0, 0, 624, 104, 0, 0, 624, 104, 0, 6, 24, 0, 0, 0, 416, 104, 0, 0, 208, 104, 0, 0, 208, 104, 0, 6, 3, 0, 0],
    (240, 1, 9, 11): [0, 64, 8, 0, 0, 512, 8, 0, 0, 960, 8, 0, 0, 960, 8, 0, 6, 240, 0, 0, 3, 45, 0, 1, -1, -1, -1, -1, 3, 45, 0, 1, 6, 240, 0, 0, 3, 45, 0, 1, 1, 48, 8, 0, 3, 27, 0, 1, 6, 120, 0, 0, 0, 512, 8, 0, 0, 64, 8, 0, 0, 64, 8, 0, 6, 3, 0, 0],
}


def wgrad_routes(lib, da, B, H, W, ncu=256):
    """[(kernel, workgroups, S, staged)] x 17"""
    out = (C.c_int * 68)()
    assert lib.sinddm_debug_wgrad_routes(da, B, H, W, ncu, out, 68) == 0
    return [tuple(out[4 * i:4 * i + 4]) for i in range(17)]


def launches(dim):
    """(taps, C_in, C_out, index of the matching data-gradient route in sinddm_debug_routes or None) of the 17 launches"""
    half = dim // 2
    cin, cout = (3, half, dim, dim), (half, dim, dim, half)
    out = [(1, half, 3, None)]
    for l in (3, 2, 1, 0):
        out += [(9, cout[l], cout[l], 8 + 2 * l), (1, cin[l], cout[l], None), (9, cin[l], cout[l], 8 + 2 * l + 1), (25, cin[l], cin[l], None)]
    return out


def ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("key", sorted(PINNED), ids=lambda k: f"dim{k[0] & 0xFFFF}{'_fp32' if k[0] & FP32 else ''}_{k[1]}x{k[2]}x{k[3]}")
def test_pinned_rows(key):
    got = wgrad_routes(_lib.load(), *key)
    assert [v for launch in got for v in launch] == PINNED[key], "17 x (kernel, workgroups, S, staged) at 256 compute units"
    assert key in set(grid())


def test_pinned_rows_show_every_kernel():
    assert {PINNED[k][4 * i] for k in PINNED for i in range(17)} == {-1, *range(8)}


def test_structure_of_the_table():
    lib = _lib.load()
    seen = set()
    wg, sp = (C.c_uint32 * 512)(), (C.c_int32 * 256)()
    for da, B, H, W in grid():
        dim = da & 0xFFFF
        routes = (C.c_int * 16)()
        assert lib.sinddm_debug_routes(da, 1, B, H, W, routes) == 0
        for ncu in NCUS:
            for (taps, cin, cout, dgrad), (kernel, nwg, S, staged) in zip(launches(dim), wgrad_routes(lib, da, B, H, W, ncu)):
                where = (da, B, H, W, ncu, taps, cin, cout)
                seen.add(kernel)
                if taps == 25:
                    assert kernel == (DW_ROWS if W % 4 == 0 and W >= 192 else DW_TILES) and (nwg, S, staged) == (cin * B, 0, 0), where
                    continue
                if taps == 1 and cin == cout:                   # identity residual: no launch
                    assert (kernel, nwg, S, staged) == (-1, -1, -1, -1), where
                    continue
                assert GENERIC <= kernel <= WINO_H16 and nwg > 0, where
                if kernel == WINO_H16:
                    assert routes[dgrad] == WH and not da & FP32 and W % 4 == 0, where
                if kernel >= WINO:
                    assert taps == 9 and (kernel != WINO) == (W % 4 == 0), where
                    ntiles = B * ceil_div(W, 16) * ceil_div(H, 4)
                    assert nwg == lib.sinddm_debug_wgrad_map(cin, cout, ntiles, ncu, wg, 512, sp, 256), where
                    assert S == 0 and staged == 1, where
                if taps == 9:
                    assert (kernel == SLAB3) == (cin < 16 and cout % 80 == 0), where
                assert (kernel == SLAB1) == (taps == 1 and cout % 80 == 0), where
                assert (kernel == GENERIC) == (cout % 80 != 0), where
                if kernel < WINO:
                    ntiles = B * ceil_div(H * W, 64) if kernel == SLAB1 else B * ceil_div(W, 32) * ceil_div(H, 2)
                    assert 8 <= S <= ceil_div(ntiles, 8) * 8 and S % 8 == 0 and nwg % S == 0, where
                    assert staged == (kernel == SLAB3), where
    assert seen == {-1, *range(8)}


def test_generic_kernel_never_takes_80_row_blocks():
    """The MT = 5 instantiations of the generic kernel are gone: no C_out % 80 == 0 launch may ask for them, whatever C_in,
    with or without a staging slab or running maxima."""
    lib = _lib.load()
    out = (C.c_int * 4)()
    n = 0
    for taps in (1, 9):
        for cout in range(80, 1041, 80):
            for cin in range(1, 1025):
                for scr, amax in ((0, 0), (1, 0), (1, 1)):
                    assert lib.sinddm_debug_wgrad_plan(taps, cin, cout, 2, 21, 37, scr, amax, 256, out) == 0
                    assert out[0] in ((SLAB1,) if taps == 1 else (SLAB3, WINO)), (taps, cin, cout, scr, amax, list(out))
                    n += 1
    # ... nor at a size whose Winograd launch table does not fit (more than 256 slabs: 13 x 22)
    assert lib.sinddm_debug_wgrad_plan(9, 1024, 1040, 16, 96, 128, 1, 1, 256, out) == 0 and out[0] == SLAB3
    assert lib.sinddm_debug_wgrad_plan(9, 960, 960, 16, 96, 128, 1, 1, 256, out) == 0 and out[0] == WINO_H16      # 12 x 20
    assert n == 2 * 13 * 1024 * 3


def test_existing_numeric_tests_cover_every_kernel():
    """Every weight-gradient kernel is gated numerically by a backward test that already exists: the union over their shapes."""
    import test_gpu_train as T
    lib = _lib.load()
    mark = [m for m in T.test_net_backward_vs_oracle_autograd.pytestmark if m.name == "parametrize"][0]
    shapes = [tuple(s) for s in mark.args[1]]
    assert "dim, B, H, W = 160, 8, 186, 248" in inspect.getsource(T.test_net_backward_binary16_convs_vs_float64)
    shapes.append((160, 8, 186, 248))
    seen = {launch[0] for s in shapes for launch in wgrad_routes(lib, *s)}
    assert set(range(GENERIC, WINO_H16 + 1)) <= seen, seen
    # ... and by a test of ONE launch on exact inputs (tests/test_gpu_wgrad_kernels.py): the union over its table, per grid
    from wgrad_util import c1_cases
    for ncu in NCUS:
        alone = set()
        for kernel, taps, cin, cout, B, H, W, scr, amax, variant in c1_cases():
            out = (C.c_int * 4)()
            assert lib.sinddm_debug_wgrad_plan(taps, cin, cout, B, H, W, scr, amax, ncu, out) == 0
            alone.add(out[0])
        assert alone == set(range(GENERIC, WINO_H16 + 1)), (ncu, alone)


def test_bad_arguments():
    lib = _lib.load()
    out = (C.c_int * 68)()
    assert lib.sinddm_debug_wgrad_routes(160, 0, 8, 8, 256, out, 68) < 0
    assert lib.sinddm_debug_wgrad_routes(161, 1, 8, 8, 256, out, 68) < 0
    assert lib.sinddm_debug_wgrad_routes(160, 1, 8, 8, 256, None, 68) < 0
    assert lib.sinddm_debug_wgrad_routes(160, 1, 8, 8, 256, out, 67) < 0
    assert lib.sinddm_debug_wgrad_routes(160, 1, 8, 8, 0, out, 68) == 0          # ncu <= 0: the device's (256 without one)
    assert list(out) == [v for launch in wgrad_routes(lib, 160, 1, 8, 8, 256) for v in launch]
    assert lib.sinddm_debug_wgrad_plan(3, 16, 80, 1, 8, 8, 1, 0, 256, out) < 0
    assert lib.sinddm_debug_wgrad_plan(9, 0, 80, 1, 8, 8, 1, 0, 256, out) < 0
    assert lib.sinddm_debug_wgrad_plan(9, 16, 80, 1, 8, 8, 1, 0, 256, None) < 0
