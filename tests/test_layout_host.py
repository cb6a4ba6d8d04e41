"""Layout conditioning (paint-to-image), everything that needs no GPU: the properties of the float64 restatement the GPU tests
measure the kernels against (tests/layout_util.py, written from the contract in include/sinddm_hip.h), and the host logic --
strengths, block sizes, the layout pyramid, the command line, refusals and the attributes' life cycle."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import layout_util as LU
from conftest import REPO
from sinddm_amd import _lib
from sinddm_amd.configs import build_diffusion
from sinddm_amd.functions import layout_blocks, _layout_pyramid, layout_strengths


def _randn(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


# ---- 1: the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,N", [(33, 50, 8), (25, 34, 16), (7, 9, 16), (67, 90, 3)])
def test_constant_offset_gives_constant_delta(H, W, N):
    """(a) A layout that differs from xp by a constant c gives D == c and U(D) == c: wrong divisors of partial blocks or
    weights that do not sum to 1 would show."""
    est = _randn((2, 3, H, W), 1)
    c = 0.3125
    D = LU.block_mean((est + c) - est, N)
    assert D.shape == (2, 3, -(-H // N), -(-W // N))
    if (H, W, N) == (7, 9, 16):
        assert D.shape[-2:] == (1, 1)
    assert np.abs(D - c).max() <= 1e-15
    for wrap in ((False, False), (True, True), (False, True)):
        assert np.abs(LU.upsample(D, N, H, W, wrap=wrap) - c).max() <= 1e-15


@pytest.mark.parametrize("H,W", [(33, 50), (7, 9)])
def test_block_size_one_is_the_identity(H, W):
    """(b) N = 1: U(D) = L - xp exactly."""
    r = _randn((2, 3, H, W), 2)
    D = LU.block_mean(r, 1)
    assert np.array_equal(D, r)
    assert np.array_equal(LU.upsample(D, 1, H, W), r)
    assert np.array_equal(LU.upsample(D, 1, H, W, wrap=(True, True)), r)


@pytest.mark.parametrize("offset", [False, True], ids=["zero_mean", "channel_offset"])
@pytest.mark.parametrize("H,W,N", [(33, 50, 8), (48, 64, 4), (48, 64, 2), (25, 34, 16), (67, 90, 8), (67, 90, 3)])
def test_one_pull_contracts_the_low_band(H, W, N, offset):
    """(c) With r = L - xp and r' = r - U(M r): ||M r'|| <= 0.75 ||M r||.  The block-averaged bilinear weights are a
    [1/8, 3/4, 1/8]-type smoothing per axis whose eigenvalues stay >= 1/4 (interior; edge rows have more weight on
    themselves): after one full-strength pull at most 3/4 of the band is left."""
    r = _randn((2, 3, H, W), 3)
    if offset:
        r = r + np.array([0.7, -0.4, 0.2])[None, :, None, None]
    Mr = LU.block_mean(r, N)
    r2 = r - LU.upsample(Mr, N, H, W)
    for b in range(2):
        ratio = np.linalg.norm(LU.block_mean(r2[b], N)) / np.linalg.norm(Mr[b])
        print(f"{H}x{W} N={N} offset={offset} sample {b}: ||M r'|| / ||M r|| = {ratio:.3f}")
        assert ratio <= 0.75


def test_wrapped_axis_commutes_with_block_shifts():
    """(d) On a wrapped axis whose size N divides, shifting r by a multiple of N shifts U(M r) by the same amount exactly."""
    H, W, N, sh = 48, 64, 8, 16
    r = _randn((3, H, W), 4)
    for axis, wrap in ((-1, (False, True)), (-2, (True, False)), (-1, (True, True))):
        U = LU.upsample(LU.block_mean(r, N), N, H, W, wrap=wrap)
        Us = LU.upsample(LU.block_mean(np.roll(r, sh, axis=axis), N), N, H, W, wrap=wrap)
        assert np.array_equal(Us, np.roll(U, sh, axis=axis))
    # ... which a clamped axis does not do
    U = LU.upsample(LU.block_mean(r, N), N, H, W)
    Us = LU.upsample(LU.block_mean(np.roll(r, sh, axis=-1), N), N, H, W)
    assert not np.array_equal(Us, np.roll(U, sh, axis=-1))


def test_halo_is_not_read_and_wraps():
    """Under a halo the block grid starts at the halo, D comes from the centre alone, and U in the halo is U of the wrapped
    centre pixel."""
    H, W, N, hx = 24, 32, 8, 16
    r = _randn((3, H, W), 5)
    ext = np.concatenate([r[..., -hx:], r, r[..., :hx]], axis=-1)
    junk = ext.copy()
    junk[..., :hx] = 99.0
    junk[..., -hx:] = -99.0
    D = LU.block_mean(junk, N, halo=(0, hx))
    assert np.array_equal(D, LU.block_mean(r, N))
    U = LU.upsample(D, N, H, W, halo=(0, hx))
    Uc = LU.upsample(D, N, H, W, wrap=(False, True))
    assert np.array_equal(U[..., hx:hx + W], Uc)
    assert np.array_equal(U[..., :hx], Uc[..., -hx:]) and np.array_equal(U[..., -hx:], Uc[..., :hx])


def test_full_strength_at_block_one_replaces_x_recon():
    """N = 1, g = 1: the step is the one whose x_recon is the layout -- the network's eps does not matter in mode 2."""
    net, d = build_diffusion("C2", dim=20, device="cpu")
    k = d.step_coefs(0, 1)
    assert k.mode == 2
    x, e1, e2, xt, L = (_randn((2, 3, 5, 7), 10 + i) for i in range(5))
    L = L[0] * 0.7
    z = np.zeros_like(x)
    outs = []
    for e in (e1, e2):
        D = LU.delta(k, L, x, e, xt, N=1)
        outs.append(LU.layout_step(k, x, e, xt, z, D, 1.0, 1))
    assert np.abs(outs[0] - np.clip(L, -1, 1)[None]).max() <= 1e-12
    assert np.abs(outs[0] - outs[1]).max() <= 1e-12
    # g = 0 is the ordinary step
    D = LU.delta(k, L, x, e1, xt, N=1)
    assert np.array_equal(LU.layout_step(k, x, e1, xt, z, D, 0.0, 1), LU.step(k, x, e1, xt, z, 1.0, 0.0))


# ---- 2: host logic --------------------------------------------------------------------------------------------------------
def test_layout_strengths():
    assert layout_strengths([5, 4, 3, 2, 1, 0], 0.5, 3) == [0.5, 0.5, 0.5, 0.0, 0.0, 0.0]
    assert layout_strengths([2, 1, 0]) == [1.0, 1.0, 1.0]
    assert layout_strengths([2, 1, 0], 0.0, 0) == [0.0, 0.0, 0.0]
    assert layout_strengths([], 1.0, 0) == []
    assert layout_strengths([9, 8], 1.0, 10) == [0.0, 0.0]
    for bad in ((1.5, 0), (-0.1, 0), (float("nan"), 0), (0.5, -1)):
        with pytest.raises(ValueError):
            layout_strengths([1, 0], *bad)


def test_layout_blocks():
    assert layout_blocks(8, 2.0, 4) == [1, 2, 4, 8]
    assert layout_blocks(8, 1.411, 5) == [max(1, int(round(8 / 1.411 ** (4 - s)))) for s in range(5)] == [2, 3, 4, 6, 8]
    assert layout_blocks(1, 1.411, 3) == [1, 1, 1]
    assert layout_blocks(64, 1.411, 1) == [64]
    for bad in ((0, 1.411, 3), (65, 1.411, 3), (8, 1.0, 3), (8, 1.411, 0)):
        with pytest.raises(ValueError):
            layout_blocks(*bad)


def test_layout_pyramid():
    sizes = [(12, 17), (25, 34), (50, 67)]
    const = torch.full((3, 50, 67), 0.375)
    for t, (h, w) in zip(_layout_pyramid(const, sizes), sizes):
        assert t.shape == (3, h, w) and t.dtype == torch.float32
        assert torch.equal(t, torch.full((3, h, w), 0.375))            # a constant image stays constant
    lay = torch.from_numpy(_randn((3, 50, 67), 6)).float().clamp(-1, 1)
    pyr = _layout_pyramid(lay, sizes)
    assert torch.equal(pyr[-1], lay)                                   # the finest size is the layout itself
    for t in pyr:
        assert float(t.min()) >= float(lay.min()) - 1e-6 and float(t.max()) <= float(lay.max()) + 1e-6
    # an integer ratio is the plain block mean
    half = _layout_pyramid(lay[:, :, :66], [(25, 33)])[0]
    ref = lay[:, :, :66].double().reshape(3, 25, 2, 33, 2).mean(dim=(2, 4)).float()
    assert float((half - ref).abs().max()) <= 1e-6
    with pytest.raises(ValueError):
        _layout_pyramid(lay, [(51, 67)])
    with pytest.raises(ValueError):
        _layout_pyramid(lay[0], sizes)


def test_command_line_flags():
    import main
    args = main.parse_args(["--mode", "paint2image"])
    assert (args.layout_down, args.layout_strength, args.layout_t_min, args.layout_scales) == (8, 1.0, 0, None)
    args = main.parse_args(["--mode", "paint2image", "--input_image", "sketch.png", "--layout_down", "12", "--layout_strength",
                            "0.5", "--layout_t_min", "20", "--layout_scales", "1", "3"])
    assert (args.input_image, args.layout_down, args.layout_strength, args.layout_t_min, args.layout_scales) == \
        ("sketch.png", 12, 0.5, 20, [1, 3])
    for bad in (["--layout_down", "0"], ["--layout_down", "65"], ["--layout_strength", "1.5"], ["--layout_strength", "-0.1"],
                ["--layout_t_min", "-1"], ["--layout_scales", "3", "1"], ["--layout_scales", "1"]):
        with pytest.raises(SystemExit):
            main.parse_args(["--mode", "paint2image"] + bad)
    # every other command line is unchanged: the new flags have defaults and touch nothing else
    a, b = main.parse_args(["--mode", "sample"]), main.parse_args(["--mode", "sample", "--layout_down", "8"])
    assert vars(a) == vars(b)


def test_new_symbols_declared_bound_and_struct_mirrors():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    lib = _lib.load()
    for name in ("sinddm_sample_chain_layout", "sinddm_layout_delta", "sinddm_reverse_step_layout"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    m = re.search(r"typedef struct sinddm_layout_opts \{(.*?)\} sinddm_layout_opts;", txt, re.S)
    assert m and re.findall(r"^\s*[\w ]+?\*?\s*(\w+);", m.group(1), re.M) == [f[0] for f in _lib.LayoutOpts._fields_] == ["layout", "down", "g", "delta"]
    assert C.sizeof(_lib.LayoutOpts) == 4 * C.sizeof(C.c_void_p)
    rs, lo = lib.sinddm_sample_chain_resample.argtypes, lib.sinddm_sample_chain_layout.argtypes
    assert list(lo[:-1]) == list(rs) and lo[-1] is C.POINTER(_lib.LayoutOpts)
    assert int(re.search(r"#define SINDDM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 3
    assert lib.sinddm_abi_version() == 3
    assert not _lib.missing_symbols()


def test_layout_entry_checks_and_refusals():
    net, d = build_diffusion("C1", dim=16, device="cpu")
    H, W = d.image_sizes[0]
    x = torch.zeros(2, 3, H, W)
    assert d.layout_maps is None and d.layout_down == {} and d.layout_strength == 1.0 and d.layout_t_min == 0
    assert d._layout_entry(0, x) is None
    d.layout_maps, d.layout_down = {0: torch.zeros(3, H, W)}, {0: 4}
    assert d._layout_entry(1, x) is None                   # no entry for that scale
    lay, N, g, t_min = d._layout_entry(0, x)
    assert lay.shape == (3, H, W) and (N, g, t_min) == (4, 1.0, 0)
    d.layout_strength, d.layout_t_min = {0: 0.25}, {0: 7}
    assert d._layout_entry(0, x)[1:] == (4, 0.25, 7)
    d.layout_strength = {1: 0.5}                           # a dict without the scale: strength 0, no conditioning
    assert d._layout_entry(0, x) is None
    d.layout_strength, d.layout_t_min = 0.0, 0
    assert d._layout_entry(0, x) is None
    d.layout_strength = 1.0
    with pytest.raises(_lib.SinddmError, match="layout_maps"):
        d._layout_entry(0, torch.zeros(2, 3, H, W + 1))
    d.layout_maps = {0: torch.zeros(3, H, W, dtype=torch.float64)}
    with pytest.raises(_lib.SinddmError, match="layout_maps"):
        d._layout_entry(0, x)
    d.layout_maps = {0: torch.zeros(3, H, W)}
    for down, strength, tm in ((0, 1.0, 0), (65, 1.0, 0), (4, 1.5, 0), (4, 0.5, -1)):
        d.layout_down, d.layout_strength, d.layout_t_min = {0: down}, strength, tm
        with pytest.raises(ValueError):
            d._layout_entry(0, x)
    d.layout_down, d.layout_strength, d.layout_t_min = {}, 1.0, 0
    with pytest.raises(ValueError):
        d._layout_entry(0, x)
    d.layout_down = {0: 4}
    # resample with R > 1: not built; R = 1 is no resampling
    d.resample = (1, 3)
    assert d._layout_entry(0, x) is not None
    d.resample = (2, 2)
    with pytest.raises(NotImplementedError):
        d._run_steps(x, 0, [3, 2, 1, 0])
    with pytest.raises(NotImplementedError):
        d._p_sample_host_t(x, 3, 0)
    d.layout_strength = 0.0                                # strength 0 is the plain resampled run: nothing to refuse
    assert d._layout_entry(0, x) is None
    d.layout_strength = 1.5                                # ... but the range is checked first
    with pytest.raises(ValueError):
        d._layout_entry(0, x)
    d.layout_strength = 1.0
    d.resample = None
    d.clip_guided_sampling = True
    with pytest.raises(NotImplementedError):
        d._run_steps(x, 0, [3, 2, 1, 0])
    with pytest.raises(NotImplementedError):
        d._p_sample_host_t(x, 3, 0)


def test_paint2image_validates_and_clears_its_attributes():
    from sinddm_amd.trainer import MultiscaleTrainer
    net, d = build_diffusion("C1", dim=16, device="cpu")
    tr = MultiscaleTrainer.__new__(MultiscaleTrainer)      # (the driver alone: no data folder, no optimiser)
    tr.ema_model, tr.n_scales, tr.scale_factor, tr.device = d, d.n_scales, d.scale_factor, "cpu"
    seen = {}

    def sample_scales(**kw):
        seen.update(maps=d.layout_maps, down=dict(d.layout_down), g=d.layout_strength, t_min=d.layout_t_min, kw=kw)
        raise RuntimeError("stop here")

    tr.sample_scales = sample_scales
    H, W = d.target_size(d.n_scales - 1, (1, 1))
    lay = torch.full((3, H, W), 0.25)
    with pytest.raises(RuntimeError, match="stop here"):
        tr.paint2image(lay, batch_size=2, down=8, strength=0.5, t_min=3, scales=(1, 2), save_images=False)
    assert sorted(seen["maps"]) == [1, 2] and seen["g"] == 0.5 and seen["t_min"] == 3
    blocks = layout_blocks(8, d.scale_factor, d.n_scales)
    assert seen["down"] == {1: blocks[1], 2: blocks[2]}
    for s in (1, 2):
        assert tuple(seen["maps"][s].shape) == (3,) + tuple(d.target_size(s, (1, 1)))
        assert torch.equal(seen["maps"][s], torch.full_like(seen["maps"][s], 0.25))
    assert seen["kw"]["batch_size"] == 2 and seen["kw"]["start_noise"] is True
    # cleared after the raise
    assert d.layout_maps is None and d.layout_down == {} and d.layout_strength == 1.0 and d.layout_t_min == 0
    for kw in (dict(layout=lay[:, :-1]), dict(layout=lay[0]), dict(layout=lay, strength=1.5), dict(layout=lay, t_min=-1),
               dict(layout=lay, down=0), dict(layout=lay, down=65), dict(layout=lay, scales=(2, 1)),
               dict(layout=lay, scales=(0, d.n_scales))):
        with pytest.raises(ValueError):
            tr.paint2image(**kw)
        assert d.layout_maps is None and d.layout_down == {}
    # a stretched canvas takes the stretched finest size
    H2, W2 = d.target_size(d.n_scales - 1, (1, 2))
    with pytest.raises(ValueError):
        tr.paint2image(lay, scale_mul=(1, 2))
    with pytest.raises(RuntimeError, match="stop here"):
        tr.paint2image(torch.zeros(3, H2, W2), scale_mul=(1, 2))
    assert tuple(seen["maps"][0].shape) == (3,) + tuple(d.target_size(0, (1, 2)))
