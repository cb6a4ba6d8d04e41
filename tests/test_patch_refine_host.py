"""CPU: the host side of the patch-vote refinement -- the three new C entries are declared, bound and exported and refuse
bad arguments before any device work; the Python validation; the command line; and the numpy references the GPU tests
are held against (tests/refine_util.py): the plain loop's energy falls, the completeness scale changes the winners, and a
float32 emulation of the scaled ranking contract stays inside the bound derived for it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nnf_util as U
import refine_util as R
from conftest import GOLDEN, REPO
from sinddm_amd import _lib

ENTRIES = ("sinddm_patch_nnf_scaled_workspace_bytes", "sinddm_patch_nnf_scaled", "sinddm_patch_vote")


@pytest.fixture(scope="module")
def crops():
    return R.inputs(GOLDEN)


def test_entries_are_declared_bound_and_exported():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.sinddm_abi_version() == _lib.ABI_VERSION == 3   # additive
    assert not _lib.missing_symbols()


def test_scaled_workspace_holds_the_query_norms():
    lib = _lib.load()
    for P, wrap in ((7, 0), (5, 3), (3, 1)):
        a = lib.sinddm_patch_nnf_workspace_bytes(2, 29, 37, 31, 41, P, wrap, 0)
        b = lib.sinddm_patch_nnf_scaled_workspace_bytes(2, 29, 37, 31, 41, P, wrap, 0)
        hq, wq = U.grid((29, 37), P, (bool(wrap & 1), bool(wrap & 2)))
        assert a > 0 and b >= a + 2 * hq * wq * 4
    assert lib.sinddm_patch_nnf_scaled_workspace_bytes(2, 29, 37, 29, 37, 4, 0, 0) == 0
    assert lib.sinddm_patch_nnf_scaled_workspace_bytes(0, 29, 37, 29, 37, 7, 0, 0) == 0
    assert lib.sinddm_patch_nnf_scaled_workspace_bytes(1, 6, 37, 29, 37, 7, 0, 0) == 0


def test_scaled_entry_refuses_before_any_device_work():
    lib = _lib.load()
    buf = (C.c_float * 16)()                                  # never dereferenced: every call below is refused
    p = C.cast(buf, C.c_void_p)
    big = 1 << 30

    def call(query=p, ref=p, scale=p, dist=p, idx=p, B=1, Hq=29, Wq=37, Hr=29, Wr=37, P=7, ws=p, ws_bytes=big):
        return lib.sinddm_patch_nnf_scaled(query, 1, ref, 0, None, scale, 0, dist, idx, B, Hq, Wq, Hr, Wr, P, 0, 0, ws,
                                           ws_bytes, None)

    for scale in (p, None):                                   # (NULL scale: the refusals of sinddm_patch_nnf itself)
        for kw in (dict(query=None), dict(ref=None), dict(dist=None), dict(idx=None), dict(ws=None), dict(B=0), dict(P=4),
                   dict(P=9), dict(ws_bytes=16)):
            assert call(scale=scale, **kw) == -1, (scale, kw)
        assert call(scale=scale, Hq=6) == -2
        assert call(scale=scale, Wr=6) == -2
        assert call(scale=scale, Hr=50000, Wr=50000) == -2
        assert call(scale=scale, Hq=4, P=5) == -2
    # a workspace that is enough for the plain search only
    plain = lib.sinddm_patch_nnf_workspace_bytes(1, 29, 37, 29, 37, 7, 0, 0)
    assert call(ws_bytes=plain) == -1


def test_vote_entry_refuses_before_any_device_work():
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)

    def call(idx=p, ref=p, base=p, out=p, B=1, Hq=29, Wq=37, Hr=29, Wr=37, P=7, blend=1.0):
        return lib.sinddm_patch_vote(idx, ref, 0, base, None, 0, out, B, Hq, Wq, Hr, Wr, P, 0, 0, blend, None)

    for kw in (dict(idx=None), dict(ref=None), dict(base=None), dict(out=None), dict(B=0), dict(B=-3), dict(P=4), dict(P=9),
               dict(P=1), dict(blend=-0.25), dict(blend=1.5), dict(blend=float("nan")), dict(blend=float("inf"))):
        assert call(**kw) == -1, kw
    for kw in (dict(Hq=6), dict(Wq=6), dict(Hr=6), dict(Wr=6), dict(Hq=4, P=5), dict(Wr=2, P=3)):
        assert call(**kw) == -2, kw


def test_python_validation():
    from sinddm_amd.metrics import check_ref_scale
    from sinddm_amd.refine import PatchRefine, check_alpha, check_blend, patch_refine, patch_vote
    E = _lib.SinddmError
    ok = torch.ones(2, 5, 6)
    assert check_ref_scale(ok, 2, (5, 6)) is ok and check_ref_scale(ok[0], 2, (5, 6)).shape == (1, 5, 6)
    for bad in (torch.zeros(5, 6), -ok, ok * float("inf"), ok * float("nan"), torch.ones(3, 5, 6), torch.ones(5, 7),
                ok.double(), [1.0]):
        with pytest.raises(E, match="ref_scale"):
            check_ref_scale(bad, 2, (5, 6))
    one_bad = ok.clone()
    one_bad[1, 4, 5] = 0.0
    with pytest.raises(E, match="finite and > 0"):
        check_ref_scale(one_bad, 2, (5, 6))
    for bad in (-0.1, 1.01, float("nan"), float("inf"), "x", None):
        with pytest.raises(E, match="blend"):
            check_blend(bad)
    assert check_blend(0) == 0.0 and check_blend(1) == 1.0 and check_blend(0.5) == 0.5
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(E, match="alpha"):
            check_alpha(bad)
    assert check_alpha(None) is None and check_alpha(0.005) == 0.005
    # the blend is judged before anything asks for a device
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(E, match="blend"):
        patch_vote(torch.zeros(1, 10, 10, dtype=torch.int32), x, (16, 16), 7, base=x, blend=2.0)
    with pytest.raises(E, match="blend"):
        patch_refine(x, x[0], blend=-1.0)
    with pytest.raises(E, match="iters"):
        patch_refine(x, x[0], iters=0)
    with pytest.raises(E, match="no CPU fallback"):
        patch_vote(torch.zeros(1, 10, 10, dtype=torch.int32), x, (16, 16), 7, base=x)
    with pytest.raises(E, match="no CPU fallback"):
        patch_refine(x, x[0])
    # the option of sample_scales
    o = PatchRefine.of(dict(iters=2, patch=5, alpha=0.01, blend=0.5, scales=(1, 3)))
    assert (o.iters, o.patch, o.alpha, o.blend, o.scales) == (2, 5, 0.01, 0.5, (1, 3))
    assert o.covers(1) and o.covers(3) and not o.covers(0) and not o.covers(4)
    assert PatchRefine.of(PatchRefine()).covers(9) and PatchRefine.of({}).iters == 1
    for bad in (dict(scales=(2, 1)), dict(scales=(-1, 2)), dict(scales=(1,)), dict(scales=(0.5, 2)), dict(iters=0),
                dict(iters=1.5), dict(patch=4), dict(alpha=0.0), dict(blend=2.0), dict(steps=3), 7):
        with pytest.raises(E, match="patch_refine"):
            PatchRefine.of(bad)


def test_unbuilt_combinations_are_named():
    from sinddm_amd.sampler import NOT_BUILT
    for other in ("keep_maps", "layout_maps", "roi"):
        assert "patch_refine" in NOT_BUILT["patch_refine", other]


def test_command_line():
    import main
    a = main.parse_args(["--mode", "sample"])
    assert a.patch_refine is None and a.patch_refine_opt is None           # off by default
    a = main.parse_args(["--mode", "sample", "--patch_refine", "2"])
    assert a.patch_refine_opt == dict(iters=2, patch=7, alpha=None, blend=1.0, scales=None)
    a = main.parse_args(["--mode", "evaluate", "--patch_refine", "1", "--patch_refine_patch", "5", "--patch_refine_alpha",
                         "0.005", "--patch_refine_blend", "0.5", "--patch_refine_scales", "2", "3"])
    assert a.patch_refine_opt == dict(iters=1, patch=5, alpha=0.005, blend=0.5, scales=(2, 3))
    for bad in (["--mode", "train", "--patch_refine", "1"], ["--mode", "inpaint", "--patch_refine", "1"],
                ["--mode", "sample", "--patch_refine", "0"], ["--mode", "sample", "--patch_refine", "1", "--patch_refine_patch", "4"],
                ["--mode", "sample", "--patch_refine", "1", "--patch_refine_alpha", "0"],
                ["--mode", "sample", "--patch_refine", "1", "--patch_refine_alpha", "nan"],
                ["--mode", "sample", "--patch_refine", "1", "--patch_refine_blend", "1.5"],
                ["--mode", "sample", "--patch_refine", "1", "--patch_refine_blend", "nan"],
                ["--mode", "sample", "--patch_refine", "1", "--patch_refine_scales", "3", "2"],
                ["--mode", "sample", "--patch_refine_alpha", "0.005"], ["--mode", "sample", "--patch_refine_scales", "0", "1"]):
        with pytest.raises(SystemExit):
            main.parse_args(bad)
    src = open(os.path.join(REPO, "main.py")).read()
    assert "--patch_refine ITERS" in src.split('"""')[1]                   # the header comment knows the flag


# ---- the references themselves ----

@pytest.mark.parametrize("blend", [1.0, 0.5])
@pytest.mark.parametrize("wrap", [(False, False), (True, True)], ids=["plain", "wrapxy"])
@pytest.mark.parametrize("P", [3, 5, 7])
def test_reference_energy_falls(crops, P, wrap, blend):
    q, r, _ = crops
    es, _, _ = R.refine64(q, r, P, 3, wrap_q=wrap, blend=blend)
    print(f"P={P} wrap={wrap} blend={blend}: E* " + " -> ".join(f"{e:.4g}" for e in es))
    assert all(b <= a for a, b in zip(es, es[1:])), es
    if blend == 1.0 and wrap == (False, False):
        # the first plain iteration of the noisy crop: the GPU test asks for a hundredth, the reference has far more room
        # (1 / 713 at P = 3, 1 / 1133 at P = 5, 1 / 1087 at P = 7)
        assert es[1] < es[0] / 500.0, es


@pytest.mark.parametrize("P", [3, 5, 7])
def test_completeness_scale_changes_the_winners(crops, P):
    q, r, wide = crops
    for ref in (r, wide):
        s = R.completeness_scale(q, ref, P)
        assert s.dtype == np.float32 and np.isfinite(s).all() and (s > 0).all()
        plain, _ = R.field64(q, ref, P)
        scaled, _ = R.field64(q, ref, P, scale=s.reshape(-1))
        share = float((plain != scaled).mean())
        print(f"P={P} ref {ref.shape[1:]}: the scale changes {share:.0%} of the winners")
        assert share >= 0.25, share


@pytest.mark.parametrize("wrap", [(False, False), (False, True)], ids=["plain", "wrapx"])
@pytest.mark.parametrize("P", [3, 5, 7])
def test_float32_emulation_of_the_scaled_ranking_is_inside_the_bound(crops, P, wrap):
    q, r, _ = crops
    s = R.completeness_scale(q, r, P, wrap_q=wrap)
    A, _ = U.patches(q, P, wrap)
    Bm, _ = U.patches(r, P)
    v = R.scaled_values_f32(A, Bm, s.reshape(-1))
    assert v.dtype == np.float32 and (v >= 0).all()
    v64, e = R.scaled_values_64(q, r, P, s, wrap_q=wrap)       # every pair, not only the winners
    worst = float((np.abs(v.astype(np.float64) - v64) / e).max())
    print(f"emulated P={P} wrap={wrap}: worst |v - v64| / e over all pairs {worst:.3f}")
    assert worst <= 1.0
    idx = v.argmin(axis=1)                                     # (argmin: of equal values the first)
    ratio = R.check_scaled_field(q, r, P, s, idx, wrap_q=wrap, what=f"emulated P={P} wrap={wrap}")
    assert ratio <= 1.0


def test_vote_reference_on_a_hand_made_field():
    P, H, W = 3, 5, 6
    rng = np.random.default_rng(0)
    ref = rng.uniform(-1, 1, (3, 7, 8)).astype(np.float32)
    base = rng.uniform(-1, 1, (3, H, W)).astype(np.float32)
    h, w = U.grid((H, W), P, (False, False))
    # every patch points at reference position (2, 3): pixel (y, x) is covered by patches whose (dy, dx) differ, so the
    # mean mixes reference pixels -- except in the corners, which one patch covers
    idx = np.full((h, w), 2 * 6 + 3)
    out = R.vote_f32(idx, ref, base, P)
    assert np.array_equal(out[:, 0, 0], ref[:, 2, 3]) and np.array_equal(out[:, H - 1, W - 1], ref[:, 4, 5])
    # no patch anywhere: the base comes back; blend 0 likewise
    assert np.array_equal(R.vote_f32(np.full((h, w), -1), ref, base, P), base)
    assert np.array_equal(R.vote_f32(idx, ref, base, P, blend=0.0), base)
    # one patch on a P x P image: the patch itself
    one = R.vote_f32(np.array([[9]]), ref, base[:, :3, :3], P)
    assert np.array_equal(one, ref[:, 1:4, 3:6])
    # float64 agrees to rounding
    assert np.allclose(out, R.vote64(idx, ref, base, P), rtol=0, atol=1e-6)
