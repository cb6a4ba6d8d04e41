"""CPU: the host side of the windowed patch search -- `refine.carry_field`, the numpy yardstick `local_util.local_field64`,
the validation of `radius` in `PatchRefine`, `patch_refine` and on the command line, and the new entry's declaration,
binding and refusals (which happen before any device work)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import local_util as L
import nnf_util as U
import refine_util as R
from conftest import GOLDEN, REPO
from sinddm_amd import _lib

PLAIN = (False, False)


@pytest.fixture(scope="module")
def crops():
    return R.inputs(GOLDEN)


def _identity(q_size, r_grid, P, wrap=PLAIN, shift=(0, 0), B=1):
    """The field y -> y + shift of samples of `q_size`, clamped into `r_grid`, (B, 2, h, w) int32."""
    h, w = U.grid(q_size, P, wrap)
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.stack([np.clip(yy + shift[0], 0, r_grid[0] - 1), np.clip(xx + shift[1], 0, r_grid[1] - 1)])
    return torch.from_numpy(np.broadcast_to(f[None], (B, 2, h, w)).astype(np.int32).copy())


# ---- carry_field ----

def test_carry_field_equal_sizes_is_the_identity():
    from sinddm_amd.refine import carry_field
    rng = np.random.default_rng(0)
    for P, wrap in ((3, PLAIN), (5, (True, False)), (7, (True, True))):
        q, r = (22, 26), (24, 30)
        h, w = U.grid(q, P, wrap)
        hr, wr = U.grid(r, P, PLAIN)
        f = torch.from_numpy(np.stack([rng.integers(0, hr, (2, h, w)), rng.integers(0, wr, (2, h, w))], 1).astype(np.int32))
        f[0, :, 3, 4] = torch.tensor([-1, wr - 1], dtype=torch.int32)      # what patch_nnf writes for "no patch"
        out = carry_field(f, P, q, q, r, r, wrap_query=wrap)
        assert out.dtype == torch.int32 and torch.equal(out, f), (P, wrap)


def test_carry_field_identity_and_shift_across_sizes():
    from sinddm_amd.refine import carry_field
    P = 5
    small, big = (22, 26), (31, 37)
    gs, gb = U.grid(small, P, PLAIN), U.grid(big, P, PLAIN)
    out = carry_field(_identity(small, gs, P), P, small, big, small, big).numpy()
    assert out.shape == (1, 2) + gb
    yy, xx = np.mgrid[0:gb[0], 0:gb[1]]
    assert np.abs(out[0, 0] - yy).max() <= 1 and np.abs(out[0, 1] - xx).max() <= 1
    # ... and down again
    back = carry_field(_identity(big, gb, P), P, big, small, big, small).numpy()
    yy2, xx2 = np.mgrid[0:gs[0], 0:gs[1]]
    assert np.abs(back[0, 0] - yy2).max() <= 1 and np.abs(back[0, 1] - xx2).max() <= 1
    # a constant shift carries to shift x ratio (where neither the old nor the new field was clamped)
    shift = (3, -4)
    out = carry_field(_identity(small, gs, P, shift=shift), P, small, big, small, big).numpy()
    ry, rx = big[0] / small[0], big[1] / small[1]
    inner = np.zeros(gb, bool)
    inner[2:gb[0] - 8, 10:gb[1] - 2] = True                                # (3 * 31 / 22 < 5, 4 * 37 / 26 < 6; + the lookup's reach)
    assert np.abs(out[0, 0] - (yy + shift[0] * ry))[inner].max() <= 1
    assert np.abs(out[0, 1] - (xx + shift[1] * rx))[inner].max() <= 1
    assert out[0, 0].min() >= 0 and out[0, 0].max() < gb[0] and out[0, 1].min() >= 0 and out[0, 1].max() < gb[1]


def test_carry_field_missing_entries_bounds_and_determinism():
    from sinddm_amd.refine import carry_field
    P = 7
    q0, q1, r0, r1 = (22, 26), (29, 35), (24, 30), (32, 40)
    g0, gr0, gr1 = U.grid(q0, P, PLAIN), U.grid(r0, P, PLAIN), U.grid(r1, P, PLAIN)
    rng = np.random.default_rng(1)
    f = np.stack([rng.integers(0, gr0[0], (3,) + g0), rng.integers(0, gr0[1], (3,) + g0)], 1).astype(np.int32)
    f[1] = np.array([-1, gr0[1] - 1], np.int32)[:, None, None]             # a whole sample without patches
    f[0, :, 0, 0] = (gr0[0] - 1, gr0[1] - 1)                               # the far corner of the old reference grid
    out = carry_field(torch.from_numpy(f), P, q0, q1, r0, r1)
    assert torch.equal(out, carry_field(torch.from_numpy(f.copy()), P, q0, q1, r0, r1))
    out = out.numpy()
    assert out.shape == (3, 2) + U.grid(q1, P, PLAIN)
    assert (out[1, 0] == -1).all() and (out[1, 1] == gr1[1] - 1).all()     # -1 stays the linear position -1
    for b in (0, 2):
        assert out[b, 0].min() >= 0 and out[b, 0].max() < gr1[0] and out[b, 1].min() >= 0 and out[b, 1].max() < gr1[1]
    # by hand for query (0, 0): u = 3.5 * 22 / 29 - 0.5 = 2.155 reads old position 0 with offset -0.845, so the old corner 17
    # goes to round((17 + 3.5 - 0.845) * 32 / 24 - 3.5) = round(22.71); in x round((23 + 3.5 - 0.9) * 40 / 30 - 3.5) = round(30.63)
    assert tuple(out[0, :, 0, 0]) == (23, 31)


def test_carry_field_wrapped_query_axis_looks_up_modulo_the_grid():
    from sinddm_amd.refine import carry_field
    P = 5
    q0, q1, r0, r1 = (20, 24), (31, 37), (20, 24), (31, 37)               # (a ratio that puts no value on a rounding tie)
    wrap = (False, True)
    g0, g1 = U.grid(q0, P, wrap), U.grid(q1, P, wrap)
    assert g0 == (16, 24) and g1 == (27, 37)
    gr0 = U.grid(r0, P, PLAIN)
    # the field's x entry names the old query column, so the result shows which column was looked up
    col = np.minimum(np.arange(g0[1]), gr0[1] - 1)
    f = np.stack([np.zeros(g0, np.int64), np.broadcast_to(col[None], g0)])[None].astype(np.int32)
    f[0, 1, :, 0] = 7                                                      # column 0 says 7: only a lookup AT column 0 sees it
    out = carry_field(torch.from_numpy(f), P, q0, q1, r0, r1, wrap_query=wrap).numpy()
    assert out.shape == (1, 2) + g1
    # the centres of the new columns in the old sample; the first one lies before old column 0 and reads column 23
    u = (np.arange(g1[1]) + 2.5) * q0[1] / q1[1] - 0.5
    looked = np.floor(u - 2 + 0.5).astype(int)
    assert looked.min() == -1
    for x_new in range(g1[1]):
        x_old = looked[x_new] % g0[1]
        want = (f[0, 1, 0, x_old] + 2.5 + (u[x_new] - looked[x_new] - 2)) * r1[1] / r0[1] - 0.5 - 2
        want = int(np.clip(np.floor(want + 0.5), 0, U.grid(r1, P, PLAIN)[1] - 1))
        assert out[0, 1, 0, x_new] == want, (x_new, x_old)


def test_carry_field_scale_mul_style_sizes():
    """A stretched sample against an unstretched image: the query and reference ratios differ per axis."""
    from sinddm_amd.refine import carry_field
    P = 5
    q0, q1, r0, r1 = (22, 52), (31, 74), (22, 26), (31, 37)               # the sample is twice as wide as the image
    gq0, gq1, gr0, gr1 = (U.grid(s, P, PLAIN) for s in (q0, q1, r0, r1))
    yy, xx = np.mgrid[0:gq0[0], 0:gq0[1]]
    f = np.stack([np.clip(yy, 0, gr0[0] - 1), np.clip(xx // 2, 0, gr0[1] - 1)])[None].astype(np.int32)
    out = carry_field(torch.from_numpy(f), P, q0, q1, r0, r1).numpy()
    assert out.shape == (1, 2) + gq1
    yy1, xx1 = np.mgrid[0:gq1[0], 0:gq1[1]]
    assert np.abs(out[0, 0] - yy1).max() <= 1
    inner = xx1 < 2 * (gr1[1] - 2)
    assert np.abs(out[0, 1] - xx1 / 2.0)[inner].max() <= 2                 # half a position of the halving, one of each rounding
    assert out[0, 1].max() < gr1[1] and out[0, 0].max() < gr1[0] and out.min() >= 0
    for bad in (dict(q_from=(4, 26)), dict(patch=4), dict(q_from=(23, 26))):
        kw = dict(patch=P, q_from=q0, q_to=q1, r_from=r0, r_to=r1)
        kw.update(bad)
        with pytest.raises(_lib.SinddmError, match="carry_field"):
            carry_field(torch.from_numpy(f), **kw)


# ---- the yardstick ----

@pytest.mark.parametrize("P", [3, 5, 7])
def test_local_field64_is_field64_when_every_window_covers_the_grid(crops, P):
    q, r, _ = crops
    hr, wr = U.grid(r.shape[1:], P, PLAIN)
    M = np.prod(U.grid(q.shape[1:], P, PLAIN))
    centre = np.full(M, (hr // 2) * wr + wr // 2)
    full_idx, full_D = R.field64(q, r, P)
    idx, D = L.local_field64(q, r, P, centre, max(hr, wr), PLAIN, PLAIN)
    assert np.array_equal(idx, full_idx) and np.array_equal(D, full_D)
    # wrapped reference axes: any prior, a radius of half the grid
    hw, ww = U.grid(r.shape[1:], P, (True, True))
    prior = np.random.default_rng(P).integers(0, hw * ww, M)
    full_idx, full_D = R.field64(q, r, P, wrap_r=(True, True))
    idx, D = L.local_field64(q, r, P, prior, 15, wrap_r=(True, True))
    assert np.array_equal(idx, full_idx) and np.array_equal(D, full_D)
    # with ok and scale
    valid = np.ones(r.shape[1:], np.float32)
    valid[8:15, 11:20] = 0.0
    ok = U.position_ok(valid, P)
    s = R.completeness_scale(q, r, P).reshape(-1)
    full_idx, _ = R.field64(q, r, P, ok=ok, scale=s)
    idx, _ = L.local_field64(q, r, P, centre, max(hr, wr), ok=ok, scale=s)
    assert np.array_equal(idx, full_idx)


def test_local_field64_windows(crops):
    q, r, _ = crops
    P = 5
    hr, wr = U.grid(r.shape[1:], P, PLAIN)
    m = L.window_mask([0, hr * wr - 1, 3 * wr + 4, -1, hr * wr], 2, (hr, wr))
    assert m.sum(axis=1).tolist() == [9, 9, 25, 0, 0]                      # clipped corners, a whole window, no prior
    m = L.window_mask([0], 2, (hr, wr), (True, True))
    assert m.sum() == 25 and m.reshape(hr, wr)[hr - 2, wr - 1]
    m = L.window_mask([5], 16, (3, 40), (True, False))                     # a wrapped window that folds onto itself
    assert m.sum() == 3 * 22
    M = np.prod(U.grid(q.shape[1:], P, PLAIN))
    prior = np.random.default_rng(0).integers(0, hr * wr, M)
    prior[:3] = (-1, hr * wr, 2 ** 31 - 1)
    idx, D = L.local_field64(q, r, P, prior, 0)
    assert (idx[:3] == -1).all() and np.array_equal(idx[3:], prior[3:])    # R = 0 evaluates the prior itself
    full = R.field64(q, r, P)[1]
    assert np.array_equal(D[np.arange(3, M), prior[3:]], full[np.arange(3, M), prior[3:]])


# ---- validation ----

def test_radius_validation():
    import main
    from sinddm_amd.metrics import check_radius, patch_nnf_local
    from sinddm_amd.refine import PatchRefine, patch_refine
    E = _lib.SinddmError
    o = PatchRefine.of({"radius": 4})
    assert o.radius == 4 and PatchRefine.of({}).radius is None and PatchRefine.of({"radius": 0}).radius == 0
    assert PatchRefine.of(PatchRefine(radius=16)).radius == 16
    for bad in (-1, 17, 2.5, "4", True):
        with pytest.raises(E, match="radius"):
            PatchRefine.of({"radius": bad})
        with pytest.raises(E, match="radius"):
            check_radius(bad)
    x = torch.zeros(1, 3, 16, 16)
    for bad in (-1, 17, 2.5):                                              # judged before anything asks for a device
        with pytest.raises(E, match="radius"):
            patch_refine(x, x[0], radius=bad)
        with pytest.raises(E, match="radius"):
            patch_nnf_local(x, x, torch.zeros(1, 10, 10, dtype=torch.int32), bad)
    with pytest.raises(E, match="prior needs a radius"):
        patch_refine(x, x[0], prior=torch.zeros(1, 10, 10, dtype=torch.int32))
    with pytest.raises(E, match="no CPU fallback"):
        patch_nnf_local(x, x, torch.zeros(1, 10, 10, dtype=torch.int32), 4)
    with pytest.raises(E, match="no CPU fallback"):
        patch_refine(x, x[0], radius=4)
    # the command line
    a = main.parse_args(["--mode", "sample", "--patch_refine", "2"])
    assert "radius" not in a.patch_refine_opt                              # absent: the option every earlier command line made
    a = main.parse_args(["--mode", "sample", "--patch_refine", "2", "--patch_refine_radius", "8"])
    assert a.patch_refine_opt == dict(iters=2, patch=7, alpha=None, blend=1.0, scales=None, radius=8)
    assert main.parse_args(["--mode", "evaluate", "--patch_refine", "1", "--patch_refine_radius", "0"]).patch_refine_opt["radius"] == 0
    for bad in (["--mode", "sample", "--patch_refine_radius", "4"],
                ["--mode", "sample", "--patch_refine", "1", "--patch_refine_radius", "-1"],
                ["--mode", "sample", "--patch_refine", "1", "--patch_refine_radius", "17"],
                ["--mode", "sample", "--patch_refine", "1", "--patch_refine_radius", "2.5"]):
        with pytest.raises(SystemExit):
            main.parse_args(bad)
    assert "--patch_refine_radius R" in open(os.path.join(REPO, "main.py")).read().split('"""')[1]


# ---- the entry ----

def test_entry_is_declared_bound_and_exported():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    name = "sinddm_patch_nnf_local"
    assert re.search(r"\b" + name + r"\s*\(", txt)
    assert name in _lib.ABI_SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == 20
    assert lib.sinddm_abi_version() == _lib.ABI_VERSION == 3               # additive
    assert not _lib.missing_symbols()


def test_entry_refuses_before_any_device_work():
    lib = _lib.load()
    buf = (C.c_float * 16)()                                               # never dereferenced: every call below is refused
    p = C.cast(buf, C.c_void_p)

    def call(query=p, ref=p, prior=p, dist=p, idx=p, scale=None, B=1, Hq=29, Wq=37, Hr=29, Wr=37, P=7, radius=4):
        return lib.sinddm_patch_nnf_local(query, 1, ref, 0, None, scale, 0, prior, radius, dist, idx, B, Hq, Wq, Hr, Wr, P, 0,
                                          0, None)

    for scale in (None, p):
        for kw in (dict(query=None), dict(ref=None), dict(prior=None), dict(dist=None), dict(idx=None), dict(B=0), dict(B=-2),
                   dict(P=4), dict(P=9), dict(P=1), dict(radius=-1), dict(radius=17)):
            assert call(scale=scale, **kw) == -1, (scale, kw)
        for kw in (dict(Hq=6), dict(Wq=6), dict(Hr=6), dict(Wr=6), dict(Hq=4, P=5), dict(Hr=50000, Wr=50000),
                   dict(Hq=50000, Wq=50000)):
            assert call(scale=scale, **kw) == -2, (scale, kw)
