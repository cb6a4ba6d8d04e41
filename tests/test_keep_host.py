"""CPU: the interface of known-region conditioning in the sampler chain (sinddm_sample_chain_keep / sinddm_reverse_step_keep:
inpainting and outpainting) -- header, ctypes binding, argument validation, the per-step forward scalars, the mask pyramid
and the placement arithmetic of `outpaint`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from sinddm_amd import _lib
from sinddm_amd.configs import CONFIGS, build_diffusion
from sinddm_amd.functions import keep_mask_pyramid, outpaint_offset

C1_HW = [(h, w) for (w, h) in CONFIGS["C1"]["sizes"]]          # (48, 64), (67, 90), (94, 126)


def test_keep_entries_declared_bound_and_opts_mirror():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    lib = _lib.load()
    for name in ("sinddm_sample_chain_keep", "sinddm_reverse_step_keep"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    m = re.search(r"typedef struct sinddm_keep_opts \{(.*?)\} sinddm_keep_opts;", txt, re.S)
    assert m, "struct sinddm_keep_opts is not in the header"
    fields = re.findall(r"const float\*\s*(\w+);", m.group(1))
    assert fields == [f[0] for f in _lib.KeepOpts._fields_] == ["mask", "x0", "ab"]
    assert C.sizeof(_lib.KeepOpts) == 3 * C.sizeof(C.c_void_p)
    # the chain entry takes every argument of sinddm_sample_chain_tile, in order, plus the keep pointer
    tile, keep = lib.sinddm_sample_chain_tile.argtypes, lib.sinddm_sample_chain_keep.argtypes
    assert list(keep[:-1]) == list(tile) and keep[-1] is C.POINTER(_lib.KeepOpts)
    # symbols were added, nothing else: the structs of the existing entries keep their layouts
    assert int(re.search(r"#define SINDDM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 3
    assert lib.sinddm_abi_version() == 3
    assert C.sizeof(_lib.StepCoefs) == 13 * 4 and C.sizeof(_lib.ChainOpts) == 3 * C.sizeof(C.c_void_p)


def test_keep_argument_validation_before_any_device_work():
    lib = _lib.load()
    one = C.cast(C.pointer(_lib.StepCoefs()), C.POINTER(_lib.StepCoefs))
    tl = (C.c_int * 1)(0)
    ab = (C.c_float * 2)(1.0, 0.0)
    flag = C.c_int(7)

    def chain(keep, x=256):
        # (fake non-null device pointers: validation returns before anything is enqueued or dereferenced)
        return lib.sinddm_sample_chain_keep(256, 256, x, 256, 256, None, one, tl, 1, 0.0, 1, 0, 160, 1, 8, 8, 256, 0, None, None,
                                            C.byref(flag), None, 0, 0, C.byref(keep) if keep is not None else None)

    def opts(mask=None, x0=None, with_ab=True):
        k = _lib.KeepOpts()
        k.mask, k.x0 = mask, x0
        if with_ab:
            k.ab = C.cast(ab, C.POINTER(C.c_float))
        return k

    assert chain(None, x=None) == -1                       # SINDDM_E_BADARG: NULL pointers
    assert chain(opts(256, 256), x=None) == -1
    assert chain(opts(mask=256)) == -1                     # mask without x0
    assert chain(opts(x0=256)) == -1                       # ... and the reverse
    assert chain(opts(256, 256, with_ab=False)) == -1      # maps without the per-step scalars
    assert chain(opts(260, 256)) == -1                     # not 16-byte aligned
    assert chain(opts(256, 264)) == -1
    assert lib.sinddm_sample_chain_keep(256, 256, 256, 256, 256, None, one, tl, 1, 0.0, 1, 0, 160, 1, 8, 8, 256, 0, None, None,
                                        C.byref(flag), None, 3, 0, C.byref(opts(256, 256))) == -1      # a halo below 16
    assert chain(opts(256, 256)) == -3                     # arguments accepted: the (empty) workspace is what fails next
    assert chain(opts()) == -3                             # no maps: `ab` is ignored, the plain call
    assert chain(None) == -3
    assert flag.value == 7

    def step(*ptrs, km=256, kx=256, ew=None, ec=None, B=1):
        x_t, eps, noise, out = ptrs
        return lib.sinddm_reverse_step_keep(x_t, eps, None, noise, out, one, ew, ec, km, kx, 1.0, 0.0, B, 3, 16, None)

    assert lib.sinddm_reverse_step_keep(None, None, None, None, None, None, None, None, None, None, 1.0, 0.0, 1, 3, 16, None) == -1
    assert step(256, 256, 256, 256, km=None) == -1 and step(256, 256, 256, 256, kx=None) == -1
    assert step(256, 256, 256, None) == -1 and step(256, 256, 256, 256, B=0) == -1
    assert step(256, 256, 256, 256, ew=256) == -1 and step(256, 256, 256, 256, ec=256) == -1        # half an edit
    mode1 = _lib.StepCoefs()
    mode1.mode = 1                                                                                      # needs x-tilde
    assert lib.sinddm_reverse_step_keep(256, 256, None, 256, 256, C.byref(mode1), None, None, 256, 256, 1.0, 0.0, 1, 3, 16,
                                        None) == -1


def test_keep_ab_table_is_the_schedule_shifted_by_one():
    """(keep_a, keep_b) of the step t -> t-1 are the registered forward tables at t-1, bit for bit; (1, 0) at t = 0."""
    net, d = build_diffusion("C1", dim=16, device="cpu")
    ab = d._keep_ab_table()
    T = d.num_timesteps
    assert ab.shape == (T, 2) and ab.dtype == np.float32 and T == CONFIGS["C1"]["T"]
    assert ab[0, 0] == np.float32(1) and ab[0, 1] == np.float32(0)
    sa, sb = d.sqrt_alphas_cumprod.numpy(), d.sqrt_one_minus_alphas_cumprod.numpy()
    for t in range(1, T):
        assert ab[t, 0].tobytes() == sa[t - 1].tobytes() and ab[t, 1].tobytes() == sb[t - 1].tobytes(), t
    assert d._keep_ab_table() is ab                        # built once per schedule
    assert d.keep_maps is None


def test_keep_maps_refuse_clip_guidance_and_mismatching_shapes():
    net, d = build_diffusion("C1", dim=16, device="cpu")
    H, W = C1_HW[0]
    x = torch.zeros(2, 3, H, W)
    d.keep_maps = {0: (torch.ones(H, W), torch.zeros(3, H, W))}
    assert d._keep_entry(1, x) is None                     # no entry for that scale
    m, k0 = d._keep_entry(0, x)
    assert m.shape == (H, W) and k0.shape == (3, H, W)
    with pytest.raises(_lib.SinddmError, match="keep_maps"):
        d._keep_entry(0, torch.zeros(2, 3, H, W + 1))
    d.keep_maps = {0: (torch.ones(H, W), torch.zeros(3, H, W, dtype=torch.float64))}
    with pytest.raises(_lib.SinddmError, match="keep_maps"):
        d._keep_entry(0, x)
    d.clip_guided_sampling = True
    with pytest.raises(NotImplementedError):
        d._run_steps(x, 0, [1, 0])
    with pytest.raises(NotImplementedError):
        d._p_sample_host_t(x, 0, 0)


def _footprint(i, n_out, n_in):
    """Input pixels [lo, hi) under output pixel i, in exact integer arithmetic."""
    return (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)


def test_keep_mask_pyramid():
    H, W = C1_HW[-1]
    ones = keep_mask_pyramid(torch.ones(H, W), C1_HW)
    zeros = keep_mask_pyramid(torch.zeros(H, W), C1_HW, hard=False)
    assert [tuple(m.shape) for m in ones] == C1_HW and all(m.dtype == torch.float32 for m in ones)
    assert all(bool((m == 1).all()) for m in ones) and all(bool((m == 0).all()) for m in zeros)
    assert all(bool((m == 1).all()) for m in keep_mask_pyramid(torch.ones(H, W), C1_HW, hard=False))
    # a 30x40 hole whose edges are no multiples of the scale ratios (94/48, 94/67)
    y0, y1, x0, x1 = 31, 61, 43, 83
    full = torch.ones(H, W)
    full[y0:y1, x0:x1] = 0
    hard, soft = keep_mask_pyramid(full, C1_HW), keep_mask_pyramid(full, C1_HW, hard=False)
    assert torch.equal(hard[-1], full) and torch.equal(soft[-1], full)         # the finest scale is the mask itself
    for (h, w), mh, ms in zip(C1_HW, hard, soft):
        assert set(mh.unique().tolist()) == {0.0, 1.0}
        assert bool((ms[mh == 1] == 1).all())                                  # hard is a subset of {soft == 1}
        touched = 0
        for i in range(h):
            lo_y, hi_y = _footprint(i, h, H)
            for j in range(w):
                lo_x, hi_x = _footprint(j, w, W)
                hits = lo_y < y1 and hi_y > y0 and lo_x < x1 and hi_x > x0
                touched += hits
                if mh[i, j] == 1:
                    assert not hits, (h, w, i, j)           # a kept pixel's footprint never touches the hole
                else:
                    assert hits, (h, w, i, j)               # ... and nothing else is given up
        assert touched > 0
    # the soft averages are the known share of the footprint: total known area is preserved
    for (h, w), ms in zip(C1_HW, soft):
        assert abs(float(ms.double().mean()) - float(full.double().mean())) < 1e-6
    with pytest.raises(ValueError):
        keep_mask_pyramid(torch.ones(3, H, W), C1_HW)


def test_outpaint_placement_arithmetic():
    net, d = build_diffusion("C1", dim=16, device="cpu")
    mul = (1, 1.5)
    want = {(0, 0): [(0, 0), (0, 0), (0, 0)],
            (0.5, 0.5): [(0, 16), (0, 22), (0, 31)],       # int(0.5 * 32), int(0.5 * 45), int(0.5 * 63)
            (1, 1): [(0, 32), (0, 45), (0, 63)]}
    for s, (h, w) in enumerate(C1_HW):
        canvas = d.target_size(s, mul)
        assert canvas == (h, int(w * 1.5))
        for anchor, offs in want.items():
            y, x = outpaint_offset(canvas, (h, w), anchor)
            assert (y, x) == offs[s], (s, anchor)
            assert 0 <= y and y + h <= canvas[0] and 0 <= x and x + w <= canvas[1]
    assert outpaint_offset((10, 10), (4, 6), (1, 0.5)) == (6, 2)
    with pytest.raises(ValueError):
        outpaint_offset(d.target_size(0, (1, 0.9)), C1_HW[0])              # scale_mul < 1 on an axis
    with pytest.raises(ValueError):
        outpaint_offset((10, 10), (4, 4), (0.5, 1.5))


def test_main_knows_the_two_modes():
    import main
    p = main.build_parser()
    a = p.parse_args(["--mode", "inpaint", "--mask_path", "hole.png", "--soft_mask"])
    assert a.mask_path == "hole.png" and a.soft_mask is True
    a = p.parse_args(["--mode", "outpaint", "--scale_mul", "1", "1.5", "--anchor", "0", "1"])
    assert a.scale_mul == [1.0, 1.5] and a.anchor == [0.0, 1.0]
    assert p.parse_args([]).anchor == [0.5, 0.5] and p.parse_args([]).soft_mask is False
    src = open(os.path.join(REPO, "main.py")).read()
    msg = re.search(r"raise NotImplementedError\((.*?)\)\n", src, re.S).group(1)
    assert "inpaint" in msg and "outpaint" in msg
