"""CPU: the routing of the 3x3 convs (conv3x3_route, sinddm_fwd.hip) as sinddm_debug_routes reports it, and the layout of the
two packed buffers (Conv3x3Images, plan.h).

Host-only hooks: without a device they assume 256 compute units, the MI355X's count -- the pinned rows below were taken at
256 CUs from the commit before the routing had one owner, the pinned layout integers from the same build.
reference: none (the reference has one convolution routine; which kernel runs is this library's own business)
"""
import ctypes as C
import itertools

import pytest

from sinddm_amd import _lib

DIMS = (10, 16, 20, 28, 32, 48, 80, 160, 240)
BATCHES = (1, 2, 4, 16, 32, 64)
SIZES = ((9, 11), (20, 20), (30, 30), (48, 64), (67, 90), (76, 95), (96, 128), (99, 130), (116, 145), (133, 177), (186, 248),
         (411, 512))
FP32 = _lib.DIM_FP32_CONVS
DIRECT, C3, WINO2, WINO3, WINO4, WH = 0, 1, 2, 3, 4, 8

# (dim_arg, B, H, W) -> (conv_path, infer_path, train_path, head_path) at 256 CUs
PINNED_ROWS = {
    (160, 64, 411, 512): (4, 8, 8, 1),
    (160, 16, 48, 64): (3, 3, 3, 1),
    (160, 16, 133, 177): (4, 8, 4, 1),
    (160, 1, 20, 20): (2, 2, 2, 1),
    (20, 4, 133, 177): (2, 2, 2, 0),
    (10, 4, 30, 30): (0, 0, 0, 0),
    (80, 16, 186, 248): (4, 8, 8, 1),
    (160 | FP32, 64, 411, 512): (4, 4, 4, 1),
}

# dim -> (sinddm_packed_count, sinddm_packed_bwd_count, sinddm_debug_head_offsets)
PINNED_LAYOUT = {
    10: (39400, 39104, (39232, 39367, 39397)),
    16: (43595, 43200, (43328, 43544, 43592)),
    20: (109965, 110784, (109632, 109902, 109962)),
    28: (118289, 118976, (117824, 118202, 118286)),
    32: (134739, 135360, (134208, 134640, 134736)),
    48: (299227, 299584, (298432, 299080, 299224)),
    80: (1740139, 1741120, (1738816, 1739896, 1740136)),
    160: (8630803, 8634176, (8628160, 8630320, 8630800)),
    240: (15286459, 15290944, (15282496, 15285736, 15286456)),
}


def routes(lib, dim_arg, train, B, H, W):
    out = (C.c_int * 16)()
    assert lib.sinddm_debug_routes(dim_arg, train, B, H, W, out) == 0
    return list(out)


def grid():
    for dim, fp32, B, (H, W) in itertools.product(DIMS, (0, FP32), BATCHES, SIZES):
        yield dim | fp32, B, H, W


@pytest.fixture(scope="module")
def table():
    """{(dim_arg, B, H, W): (inference routes, training routes)} over the whole grid, computed once."""
    lib = _lib.load()
    return {k: (routes(lib, k[0], 0, *k[1:]), routes(lib, k[0], 1, *k[1:])) for k in grid()}


def test_old_hooks_are_entry_5_of_the_new_one(table):
    lib = _lib.load()
    for (da, B, H, W), (inf, trn) in table.items():
        assert lib.sinddm_debug_infer_path(da, B, H, W) == inf[5], (da, B, H, W)
        assert lib.sinddm_debug_train_path(da, B, H, W) == trn[5], (da, B, H, W)
        assert lib.sinddm_debug_conv_path(da, B, H, W) == routes(lib, da | FP32, 1, B, H, W)[5], (da, B, H, W)
    assert len(table) == len(DIMS) * 2 * len(BATCHES) * len(SIZES)


@pytest.mark.parametrize("key", sorted(PINNED_ROWS), ids=lambda k: f"dim{k[0] & 0xFFFF}{'_fp32' if k[0] & FP32 else ''}_{k[1]}x{k[2]}x{k[3]}")
def test_pinned_rows(key):
    lib = _lib.load()
    got = (lib.sinddm_debug_conv_path(*key), lib.sinddm_debug_infer_path(*key), lib.sinddm_debug_train_path(*key),
           lib.sinddm_debug_head_path(*key))
    assert got == PINNED_ROWS[key], "(conv, infer, train, head) at 256 compute units"
    assert key in set(grid())


def test_structure_of_the_table(table):
    lib = _lib.load()
    seen_80 = 0
    for (da, B, H, W), (inf, trn) in table.items():
        dim = da & 0xFFFF
        where = (da, B, H, W)
        assert all(v in (-1, DIRECT, C3, WINO2, WINO3, WINO4, WH) for v in inf + trn), where
        assert inf[8:] == [-1] * 8, where                       # no data gradients without `train`
        assert all(v >= 0 for v in trn), where
        if (dim // 2) % 4 == 0:                                 # the plan pads rows: block 1's conv1 is the C_in = 3 kernel
            assert inf[0] == C3 and trn[0] == C3, where
        assert all(v != C3 for v in inf[1:] + trn[1:]), where
        # block 4's conv2 is missing exactly under the collapsed head
        assert (inf[7] == -1) == (lib.sinddm_debug_head_path(da, B, H, W) == 1), where
        assert all(v >= 0 for v in inf[:7]), where
        if da & FP32:
            assert WH not in inf and WH not in trn, where
        if dim == 80:
            for r in (inf, trn):
                if r[3] == WH:                                  # C_in = 40 is no multiple of 16: conv1 stays fp32
                    assert r[2] != WH, where
                    seen_80 += 1
        for l in range(4):                                      # conv1's data gradient takes conv_wh only behind conv2's
            if trn[8 + 2 * l + 1] == WH:
                assert trn[8 + 2 * l] == WH, where
    assert seen_80 > 0
    assert any(trn[8 + 2 * 2 + 1] == WH for _, trn in table.values())


@pytest.mark.parametrize("dim", DIMS)
def test_packed_layouts_do_not_move(dim):
    lib = _lib.load()
    off = (C.c_int64 * 3)()
    for da in (dim, dim | FP32):
        assert lib.sinddm_debug_head_offsets(da, off) == 0
        assert (lib.sinddm_packed_count(da), lib.sinddm_packed_bwd_count(da), tuple(off)) == PINNED_LAYOUT[dim]


def test_bad_arguments():
    lib = _lib.load()
    out = (C.c_int * 16)()
    assert lib.sinddm_debug_routes(160, 0, 0, 8, 8, out) < 0
    assert lib.sinddm_debug_routes(161, 0, 1, 8, 8, out) < 0
    assert lib.sinddm_debug_routes(160, 0, 1, 8, 8, None) < 0
