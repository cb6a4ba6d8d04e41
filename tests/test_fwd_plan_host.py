"""CPU: the plan of one network evaluation (forward_plan, csrc/fwd_plan.h) as sinddm_debug_forward_plan reports it.

Host-only hook, asked for 64, 256 and 304 compute units in both modes over the grid of test_routes_host.py.  The pinned
values (routes, head, workspace bytes) were taken at 256 CUs from the commit before the forward had a plan, through the
hooks it keeps: sinddm_debug_routes, sinddm_debug_head_path, sinddm_workspace_bytes.
reference: none (which kernels an evaluation launches and how it lays out its scratch is this library's own business)
"""
import ctypes as C

import pytest

from sinddm_amd import _lib
from test_routes_host import C3, DIRECT, FP32, WH, grid, routes

NCUS = (256, 64, 304)
N_INTS, BLOCK0, BLOCK_INTS = 80, 24, 14
TOP = ("Wp", "padded", "Wt", "HW", "head", "any_wh", "fuse_tail", "rows_aligned", "last_eps", "gx_eps", "last_fused", "gx_fused",
       "n_launches", "conv_items", "off_cond", "off_amax", "off_buf0", "off_buf1", "off_buf2", "off_buf3", "off_xpad", "core_bytes",
       "ws_bytes", "ncu")
BLK = ("route1", "route2", "variant1", "variant2", "amax_dw", "amax_in1", "amax_out1", "max_pass", "amax_in2", "resid",
       "bias_plain", "dw", "dw_pi", "dw_po")
HEAD_STEP_PITCH, HEAD_STEP, HEAD_EPS, FINAL_STEP_PITCH, FINAL_PITCH, FINAL_STEP, FINAL = range(7)
RESID_NONE, RESID_IDENTITY, RESID_FUSED, RESID_1X1 = range(4)

# (dim_arg, B, H, W) -> (head, inference routes, workspace bytes) at 256 CUs: the PINNED_ROWS keys of test_routes_host.py ...
PINNED = {
    (160, 64, 411, 512): (1, [1, 8, 8, 8, 8, 8, 8, -1], 34482151424),
    (160, 16, 48, 64): (1, [1, 3, 3, 3, 3, 3, 3, -1], 130798592),
    (160, 16, 133, 177): (1, [1, 4, 8, 8, 8, 8, 4, -1], 990148352),
    (20, 4, 133, 177): (0, [1, 0, 0, 2, 2, 2, 2, 0], 30826240),
    (10, 4, 30, 30): (0, [1, 0, 0, 0, 0, 0, 0, 0], 925440),
    (80, 16, 186, 248): (1, [1, 2, 2, 8, 8, 8, 2, -1], 947213312),
    (160 | FP32, 64, 411, 512): (1, [1, 4, 4, 4, 4, 4, 4, -1], 34482151424),
}
# ... and six tiny shapes (the GPU tests of the plan run on these): head and plain rows, head and padded rows, final conv
# with a fused tail, final conv without one, head at dim 20, head and padded rows at dim 80
TINY = {
    (160, 1, 20, 20): (1, [1, 2, 2, 2, 2, 2, 2, -1], 5993216),
    (160, 2, 9, 11): (1, [1, 2, 2, 2, 2, 2, 2, -1], 5524992),
    (20, 2, 8, 10): (0, [1, 0, 0, 2, 2, 2, 2, 0], 744192),
    (20, 2, 9, 11): (0, [1, 0, 0, 2, 2, 2, 2, 0], 756480),
    (20, 2, 8, 12): (1, [1, 0, 0, 2, 2, 2, 2, -1], 754432),
    (80, 2, 9, 11): (1, [1, 2, 2, 2, 2, 2, 2, -1], 2790912),
}
PINNED.update(TINY)


def plan(lib, dim_arg, train, B, H, W, ncu=256):
    """The hook's integers as a dict; "blk" = the four blocks' dicts, "routes" = the eight routes in launch order."""
    out = (C.c_int64 * N_INTS)()
    assert lib.sinddm_debug_forward_plan(dim_arg, train, B, H, W, ncu, out, N_INTS) == 0
    p = dict(zip(TOP, out[:BLOCK0]))
    p["blk"] = [dict(zip(BLK, out[BLOCK0 + l * BLOCK_INTS:BLOCK0 + (l + 1) * BLOCK_INTS])) for l in range(4)]
    p["routes"] = [b[k] for b in p["blk"] for k in ("route1", "route2")]
    return p


def launch_counts(p):
    """What the profiler must count in one evaluation of plan p: {kernel generation: Winograd 3x3 launches}, 1x1, direct."""
    gen = {g: sum(r == g for r in p["routes"]) for g in (8, 4, 3, 2)}
    return gen, sum(b["resid"] == RESID_1X1 for b in p["blk"]), sum(r == DIRECT for r in p["routes"])


@pytest.mark.parametrize("key", sorted(PINNED), ids=lambda k: f"dim{k[0] & 0xFFFF}{'_fp32' if k[0] & FP32 else ''}_{k[1]}x{k[2]}x{k[3]}")
def test_pinned_rows(key):
    p = plan(_lib.load(), key[0], 0, *key[1:])
    assert (p["head"], p["routes"], p["ws_bytes"]) == PINNED[key], "(head, routes, workspace bytes) at 256 compute units"


def test_agrees_with_the_older_hooks_at_256():
    lib = _lib.load()
    for da, B, H, W in list(grid()) + sorted(TINY):
        inf, trn = plan(lib, da, 0, B, H, W), plan(lib, da, 1, B, H, W)
        assert inf["routes"] == routes(lib, da, 0, B, H, W)[:8], (da, B, H, W)
        assert trn["routes"] == routes(lib, da, 1, B, H, W)[:8], (da, B, H, W)
        assert inf["head"] == lib.sinddm_debug_head_path(da, B, H, W) and trn["head"] == 0, (da, B, H, W)
        assert inf["ws_bytes"] == lib.sinddm_workspace_bytes(da, B, H, W) and trn["ws_bytes"] == 0, (da, B, H, W)
    assert set(TINY) <= set(PINNED) and all(k in set(grid()) for k in PINNED if k not in TINY)


def check_structure(p, dim_arg, train, B, H, W, ncu):
    where = (dim_arg, train, B, H, W, ncu)
    dim = dim_arg & 0xFFFF
    cout = (dim // 2, dim, dim, dim // 2)
    assert p["ncu"] == ncu and p["HW"] == H * W, where
    # geometry: training never pads; padded rows are the next multiple of 4 and carry the true width
    assert p["padded"] == (p["Wp"] != W) and p["Wt"] == (W if p["padded"] else 0), where
    assert p["Wp"] == (-(-W // 4) * 4 if p["padded"] else W) and not (train and p["padded"]), where
    assert p["fuse_tail"] == ((H * W) % 4 == 0 or p["padded"]), where
    assert p["rows_aligned"] == ((H * W) % 4 == 0 and not p["padded"]), where
    if p["head"]:
        assert p["Wp"] % 4 == 0 and not train, where
    assert (p["routes"][7] == -1) == bool(p["head"]) and all(r >= 0 for r in p["routes"][:7]), where
    assert p["any_wh"] == (WH in p["routes"]), where
    # the last launch follows (head, padded, fuse); the two arms of padded rows without the head never occur in this build
    assert p["last_eps"] == (HEAD_EPS if p["head"] else FINAL_PITCH if p["padded"] else FINAL), where
    fused = ((HEAD_STEP_PITCH if p["padded"] else HEAD_STEP) if p["head"] else FINAL_STEP_PITCH if p["padded"]
             else FINAL_STEP if p["fuse_tail"] else FINAL)
    assert p["last_fused"] == fused, where
    assert FINAL_STEP_PITCH not in (p["last_eps"], p["last_fused"]) and FINAL_PITCH not in (p["last_eps"], p["last_fused"]), where
    quads = -(-(H * (p["Wp"] // 4)) // 256)
    assert p["gx_eps"] == (quads if p["head"] or p["padded"] else -(-(-(-H * W // 4)) // 256)), where
    assert p["gx_fused"] == (quads if p["head"] or p["padded"] else -(-(H * W // 4) // 256) if p["fuse_tail"] else p["gx_eps"]), where
    # running maxima: a conv reads a slot only if exactly one earlier launch of the plan publishes it
    published, n = [], int(p["any_wh"]) + int(p["padded"]) + 1
    for l, b in enumerate(p["blk"]):
        if b["amax_dw"] >= 0:
            published.append(b["amax_dw"])
        if b["amax_in1"] >= 0:
            assert b["route1"] == WH and published.count(b["amax_in1"]) == 1 and b["amax_in1"] == 2 * l, where
        assert (b["route1"] == WH) == (b["amax_in1"] >= 0) == (b["amax_dw"] >= 0) == bool(b["bias_plain"]), where
        if b["amax_out1"] >= 0:
            assert b["route1"] in (WH, C3), where
            published.append(b["amax_out1"])
        if b["max_pass"]:
            assert b["amax_out1"] < 0 and b["amax_in2"] >= 0, where
            published.append(b["amax_in2"])
        assert (b["route2"] == WH) == (b["amax_in2"] >= 0), where
        if b["amax_in2"] >= 0:
            assert published.count(b["amax_in2"]) == 1 and b["amax_in2"] == 2 * l + 1, where
        # the 160-channel kernel: never in training; in inference exactly where C_out % 160 == 0 on conv_wh at the floor of
        # 12 items of 8x32 pixels x 160 channels per compute unit (SINDDM_WR_MIN_ITEMS_PER_CU)
        items160 = B * -(-p["Wp"] // 32) * -(-H // 8) * (cout[l] // 160)
        for r, v in ((b["route1"], b["variant1"]), (b["route2"], b["variant2"])):
            if r != WH:
                assert v == 0, where
            elif train:
                assert v == 1, where
            else:
                assert v == (2 if cout[l] % 160 == 0 and items160 >= 12 * ncu else 1), where
        # the residual: none only for block 4 under the head, identity only for the dim -> dim block
        assert (b["resid"] == RESID_NONE) == (b["route2"] < 0) and (b["resid"] == RESID_IDENTITY) == (l == 2), where
        if b["resid"] == RESID_FUSED:
            assert b["route2"] == DIRECT, where
        if b["resid"] == RESID_1X1:
            assert b["route2"] not in (DIRECT, -1), where
        assert b["dw_pi"] == b["dw_po"] == p["Wp"] and b["dw"] == int(p["Wp"] % 4 == 0 and p["Wp"] >= 192), where
        n += 2 + int(b["max_pass"]) + int(b["route2"] >= 0) + int(b["resid"] == RESID_1X1)
    assert len(set(published)) == len(published), where
    assert p["n_launches"] == n, where
    if dim == 160:
        # 14 launches under the head (+ the memset of the maxima, + the row-pad copy of padded rows), else 16
        extra = int(p["any_wh"]) + int(p["padded"])
        assert p["n_launches"] - extra == (14 if p["head"] else 16) and not any(b["max_pass"] for b in p["blk"]), where
    assert p["conv_items"] == B * -(-p["Wp"] // 32) * -(-H // 8) * 2, where
    # the workspace: regions in today's order, 256-byte aligned, disjoint, ending at core_bytes
    if train:
        assert all(p[k] == 0 for k in TOP[14:23]), where
        return
    amax = -(-B * 8 * 4 // 256) * 256
    act = -(-B * dim * H * p["Wp"] * 4 // 256) * 256
    xpad = -(-B * 3 * H * p["Wp"] * 4 // 256) * 256 if p["padded"] else 0
    offs = [p[k] for k in TOP[14:22]]
    assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and offs[0] == 0, where
    assert offs[1] >= max(B, 1024) * sum((3, dim // 2, dim, dim)) * 4, where           # the conditioning rows fit in front
    assert offs[2] - offs[1] == amax and [offs[i + 1] - offs[i] for i in range(2, 6)] == [act] * 4, where
    assert offs[7] - offs[6] == xpad, where


def test_structure_and_dependence_on_ncu():
    lib = _lib.load()
    route_moves = 0
    for da, B, H, W in list(grid()) + sorted(TINY):
        for train in (0, 1):
            ps = {ncu: plan(lib, da, train, B, H, W, ncu) for ncu in NCUS}
            for ncu, p in ps.items():
                check_structure(p, da, train, B, H, W, ncu)
            route_moves += ps[64]["routes"] != ps[304]["routes"]
            for k in ("Wp", "head", "ws_bytes", "core_bytes", "fuse_tail", "rows_aligned", "last_eps", "last_fused"):
                assert ps[64][k] == ps[256][k] == ps[304][k], (da, train, B, H, W, k)
    assert route_moves > 0


def test_the_interesting_plans_occur():
    """The structure test would pass on a grid that never reaches an arm: each one it describes is seen at 256 CUs."""
    lib = _lib.load()
    seen = set()
    for da, B, H, W in list(grid()) + sorted(TINY):
        for train in (0, 1):
            p = plan(lib, da, train, B, H, W)
            seen |= {("last", p["last_eps"]), ("last", p["last_fused"]), ("padded", p["padded"]), ("head", p["head"])}
            for b in p["blk"]:
                seen |= {("variant", b["variant1"]), ("variant", b["variant2"]), ("resid", b["resid"]), ("max_pass", b["max_pass"]),
                         ("dw", b["dw"]), ("c3 publishes", b["route1"] == C3 and b["amax_out1"] >= 0)}
    assert {("last", v) for v in (HEAD_STEP_PITCH, HEAD_STEP, HEAD_EPS, FINAL_STEP, FINAL)} <= seen
    assert {("variant", 0), ("variant", 1), ("variant", 2), ("max_pass", 1), ("dw", 0), ("dw", 1), ("c3 publishes", True)} <= seen
    assert {("resid", v) for v in range(4)} <= seen and {("padded", 1), ("head", 0), ("head", 1)} <= seen


def test_bad_arguments():
    lib = _lib.load()
    out = (C.c_int64 * N_INTS)()
    assert lib.sinddm_debug_forward_plan(160, 0, 1, 8, 8, 256, out, N_INTS) == 0
    assert lib.sinddm_debug_forward_plan(160, 0, 1, 8, 8, 256, None, N_INTS) < 0
    assert lib.sinddm_debug_forward_plan(160, 0, 1, 8, 8, 256, out, N_INTS - 1) < 0
    assert lib.sinddm_debug_forward_plan(160, 0, 0, 8, 8, 256, out, N_INTS) < 0
    assert lib.sinddm_debug_forward_plan(160, 0, 1, 0, 8, 256, out, N_INTS) < 0
    assert lib.sinddm_debug_forward_plan(160, 0, 1, 8, -1, 256, out, N_INTS) < 0
    assert lib.sinddm_debug_forward_plan(161, 0, 1, 8, 8, 256, out, N_INTS) < 0
    assert lib.sinddm_debug_forward_plan(160, 1, 1, 8, 8, 0, out, N_INTS) == 0 and out[23] == 256     # ncu <= 0: the device's
