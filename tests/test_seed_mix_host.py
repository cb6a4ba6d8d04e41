"""Seed blending on the host (no GPU): the helpers that build the blend tables (`interp_seeds`, `loop_seeds`,
`mix_from_scale`), the validation of `MultiScaleGaussianDiffusion.seed_mix`, the cut of the tables per rank, the argument
checks of sinddm_sample_chain_mix before any device work -- through the library on fake pointers, and line by line in a
stand-alone program under the address and undefined-behaviour sanitizers -- and the GIF writer."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from sinddm_amd import _lib
from sinddm_amd import dist as sdist
from sinddm_amd.models import (MIX_TOL, MultiScaleGaussianDiffusion, _check_mix, interp_seeds, loop_seeds, mix_from_scale)
from test_batch_maps_host import REPO, _host_cxx

BADARG, BADSHAPE, WORKSPACE = -1, -2, -3
P = 4096                                                                 # a fake device pointer, 16-byte aligned


def _norm_err32(row):
    w = np.asarray(row, dtype=np.float32)
    return abs(float(np.sum(w * w, dtype=np.float32)) - 1.0)


# ---- the helpers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [2, 5, 16])
def test_interp_seeds_walks_a_quarter_circle(frames):
    keys, w = interp_seeds(11, 22, frames)
    assert keys == [[11, 22]] * frames and len(w) == frames
    assert w[0] == [1.0, 0.0] and w[-1] == [0.0, 1.0]                     # the end rows: exact
    for i, row in enumerate(w):
        assert _norm_err32(row) <= 1e-6
        th = i / (frames - 1) * math.pi / 2
        assert abs(row[0] - math.cos(th)) < 1e-15 and abs(row[1] - math.sin(th)) < 1e-15
    assert all(a[0] > b[0] for a, b in zip(w, w[1:]))                     # monotone from A to B
    with pytest.raises(ValueError):
        interp_seeds(1, 2, 1)
    with pytest.raises(ValueError):
        interp_seeds(-1, 2, 4)
    with pytest.raises(ValueError):
        interp_seeds(1, 1 << 63, 4)


@pytest.mark.parametrize("frames,radius", [(8, 0.5), (16, 0.5), (3, 1.0), (5, 0.0)])
def test_loop_seeds_closes(frames, radius):
    keys, w = loop_seeds(1, 2, 3, frames, radius)
    assert keys == [[1, 2, 3]] * frames and len(w) == frames
    for i, row in enumerate(w):
        assert _norm_err32(row) <= 1e-6
        assert row[0] == math.sqrt(1 - radius * radius)
        ph = 2 * math.pi * i / frames
        assert abs(row[1] - radius * math.cos(ph)) < 1e-15 and abs(row[2] - radius * math.sin(ph)) < 1e-15
    # periodic: frame `frames` of a longer table is frame 0 -- the step from the last frame to the first is the step between
    # any two neighbours
    step = lambda a, b: math.sqrt(sum((x - y) ** 2 for x, y in zip(a, b)))
    steps = [step(w[i], w[(i + 1) % frames]) for i in range(frames)]
    assert max(steps) - min(steps) < 1e-12
    _, w2 = loop_seeds(1, 2, 3, 2 * frames, radius)
    assert all(step(w2[2 * i], w[i]) < 1e-12 for i in range(frames))      # (the same circle at twice the rate)
    assert w[0][1:] == [radius, 0.0]
    with pytest.raises(ValueError):
        loop_seeds(1, 2, 3, 8, 1.5)
    with pytest.raises(ValueError):
        loop_seeds(1, 2, 3, 0)


def test_mix_from_scale_shape_and_content():
    mix = loop_seeds(7, 8, 9, 4, 0.5)
    keys, w = mix_from_scale(mix, 2, 5)
    assert len(keys) == len(w) == 5 and all(len(t) == 4 and all(len(r) == 3 for r in t) for t in keys + w)
    for s in range(5):
        assert keys[s] == mix[0]
        assert w[s] == ([[1.0, 0.0, 0.0]] * 4 if s < 2 else mix[1])
    assert mix_from_scale(mix, 0, 3)[1] == [mix[1]] * 3
    assert mix_from_scale(mix, 3, 3)[1] == [[[1.0, 0.0, 0.0]] * 4] * 3
    keys[0][0][0] = 99                                                     # (the tables are copies)
    assert mix[0][0][0] == 7
    with pytest.raises(ValueError):
        mix_from_scale(mix, 4, 3)
    with pytest.raises(ValueError):
        mix_from_scale(([[1, 2]], [[1.0, 1.0]]), 0, 3)                    # (not unit variance)


# ---- validation -----------------------------------------------------------------------------------------------------------------
class _D:
    """What `_mix_for` / `_seeds_for` read of a MultiScaleGaussianDiffusion."""
    n_scales = 3
    noise_fn = None
    sample_seeds = None
    clip_guided_sampling = False
    seed_mix = None
    _mix_for = MultiScaleGaussianDiffusion._mix_for
    _seeds_for = MultiScaleGaussianDiffusion._seeds_for


def test_seed_mix_validation():
    d = _D()
    assert d._mix_for(0, 4) is None
    d.seed_mix = interp_seeds(1, 2, 4)
    keys, w = d._mix_for(2, 4)
    assert keys == [[1, 2]] * 4 and w == interp_seeds(1, 2, 4)[1]
    d.seed_mix = (np.array(keys), torch.tensor(w, dtype=torch.float64))   # arrays and tensors are taken too
    assert d._mix_for(0, 4)[0] == keys
    per_scale = mix_from_scale(interp_seeds(1, 2, 4), 1, 3)
    d.seed_mix = per_scale
    assert d._mix_for(0, 4)[1] == [[1.0, 0.0]] * 4 and d._mix_for(1, 4)[1] == w
    assert d._mix_for(7, 4)[1] == w                                       # (past the pyramid: the finest scale's table)
    bad = [
        (([[1, 2]] * 3, [[1.0, 0.0]] * 3), "rows for a batch of 4"),
        (([[1, -2]] * 4, [[1.0, 0.0]] * 4), "a negative seed"),
        (([[1, 1 << 63]] * 4, [[1.0, 0.0]] * 4), "a seed past 2^63"),
        (([[1, 2.5]] * 4, [[1.0, 0.0]] * 4), "a seed that is no int"),
        (([[1, 2]] * 4, [[1.0, float("nan")]] * 4), "a weight that is not finite"),
        (([[1, 2]] * 4, [[float("inf"), 0.0]] * 4), "an infinite weight"),
        (([[1, 2]] * 4, [[1.0, 0.01]] * 4), "sum w^2 = 1.0001"),
        (([[1, 2]] * 4, [[0.7, 0.7]] * 4), "sum w^2 = 0.98"),
        (([[1, 2, 3, 4, 5]] * 4, [[1.0, 0.0, 0.0, 0.0, 0.0]] * 4), "K = 5"),
        (([[]] * 4, [[]] * 4), "K = 0"),
        (([[1, 2]] * 4, [[1.0]] * 4), "rows of different length"),
        (([[1, 2]] * 4, [[1.0, 0.0]] * 3), "tables of different length"),
        ((per_scale[0][:2], per_scale[1][:2]), "two tables for three scales"),
        (([[1, 2]] * 4,), "no pair"),
    ]
    for mx, what in bad:
        d.seed_mix = mx
        with pytest.raises(ValueError):
            d._mix_for(0, 4)
            pytest.fail(what)
    d.seed_mix = ([[1, 2]] * 4, [[1.0, math.sqrt(0.9e-5)]] * 4)           # inside the tolerance
    assert abs(1.0 + 0.9e-5 - 1.0) <= MIX_TOL and d._mix_for(0, 4) is not None
    # two noise sources
    d.seed_mix = interp_seeds(1, 2, 4)
    d.sample_seeds = [1, 2, 3, 4]
    with pytest.raises(ValueError):
        d._mix_for(0, 4)
    with pytest.raises(ValueError):
        d._seeds_for(0, 4)
    d.sample_seeds, d.noise_fn = None, (lambda *a: None)
    with pytest.raises(ValueError):
        d._mix_for(0, 4)
    d.noise_fn, d.clip_guided_sampling = None, True
    with pytest.raises(NotImplementedError):
        d._mix_for(0, 4)


def test_check_mix_returns_plain_lists():
    keys, w = _check_mix(np.array([[3, 4]], dtype=np.int64), np.array([[0.6, 0.8]]))
    assert keys == [[3, 4]] and w == [[0.6, 0.8]] and all(type(v) is int for v in keys[0]) and all(type(v) is float for v in w[0])


# ---- the cut per rank -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,world", [(5, 2), (16, 3), (4, 4)])
def test_shard_rows_cuts_the_tables_like_seeds(B, world, monkeypatch):
    keys, w = loop_seeds(1, 2, 3, B, 0.5)
    keys = [[k[0] + b, k[1], k[2]] for b, k in enumerate(keys)]           # (rows that can be told apart)
    seeds = list(range(100, 100 + B))
    got_k, got_w, got_s = [], [], []
    for rank in range(world):
        monkeypatch.setattr(sdist, "rank", lambda r=rank: r)
        monkeypatch.setattr(sdist, "world_size", lambda: world)
        part_k, part_w, mine = sdist.shard_rows(keys), sdist.shard_rows(w), sdist.shard_seeds(seeds)
        assert len(part_k) == len(part_w) == len(mine) == sdist.local_batch(B)
        assert [k[0] - 1 + 100 for k in part_k] == mine                   # the rows of the samples whose seeds the rank would take
        got_k += part_k
        got_w += part_w
        got_s += mine
    assert got_k == keys and got_w == w and got_s == seeds                # in order, nothing lost


def test_driver_hook_validates_and_cuts_the_global_rows(monkeypatch):
    """`MultiscaleTrainer._local_mix`, the hook every driver with `seed_mix=` goes through: global rows in, this rank's out."""
    from sinddm_amd.trainer import MultiscaleTrainer

    class _T:
        n_scales = 3
    hook = lambda *a, **k: MultiscaleTrainer._local_mix(_T(), *a, **k)
    mix = interp_seeds(1, 2, 5)
    assert hook(None, None, 5, True) is None
    assert hook(mix, None, 5, False) == mix
    assert hook((np.array(mix[0]), torch.tensor(mix[1], dtype=torch.float64)), None, 5, False) == mix
    per_scale = mix_from_scale(mix, 1, 3)
    monkeypatch.setattr(sdist, "world_size", lambda: 2)
    monkeypatch.setattr(sdist, "rank", lambda: 1)
    o, n = sdist.shard_offset(5), sdist.local_batch(5)
    assert (o, n) == (3, 2)
    assert hook(mix, None, 5, True) == (mix[0][o:], mix[1][o:])
    assert hook(mix, None, 5, False) == mix                              # (a driver that does not shard)
    got = hook(per_scale, None, 5, True)
    assert got == ([t[o:] for t in per_scale[0]], [t[o:] for t in per_scale[1]])
    for bad in ((mix, [1, 2, 3, 4, 5]), (interp_seeds(1, 2, 4), None), ((mix[0], [[0.7, 0.7]] * 5), None),
                ((per_scale[0][:2], per_scale[1][:2]), None), ((mix[0],), None)):
        with pytest.raises(ValueError):
            hook(bad[0], bad[1], 5, True)


# ---- chain_check through the library -------------------------------------------------------------------------------------------
def _call(mix=None, seeds=None, noise=None, B=4, H=8, W=8, entry="sinddm_sample_chain_mix"):
    """The entry on fake pointers and an empty workspace; mix = (keys, weights, K) of a block, "null" for no block."""
    lib = _lib.load()
    coefs = (_lib.StepCoefs * 2)()
    tl = (C.c_int * 2)(1, 0)
    flag = C.c_int(7)
    opts = _lib.ChainOpts(None, None, noise)
    args = [P, P, P, P, P, P, coefs, tl, 2, 0.0, 1, 0, 160, B, H, W, P, 0, None, None, C.byref(flag), C.byref(opts), 0, 0, None, seeds,
            None, None, None, None]
    if entry == "sinddm_sample_chain_mix":
        args.append(None if mix == "null" else C.byref(_lib.MixOpts(*mix)))
    rc = getattr(lib, entry)(*args)
    assert flag.value == 7                                               # nothing was run
    return rc


MIX_DEFECTS = [
    ("K = 0", dict(mix=(P, P, 0)), BADARG),
    ("K = 5", dict(mix=(P, P, 5)), BADARG),
    ("keys without weights", dict(mix=(P, None, 2)), BADARG),
    ("keys off 8 bytes", dict(mix=(P + 4, P, 2)), BADARG),
    ("weights off 4 bytes", dict(mix=(P, P + 2, 2)), BADARG),
    ("a block beside sample_seeds", dict(mix=(P, P, 2), seeds=P), BADARG),
    ("more than 65535 samples", dict(mix=(P, P, 2), B=70000), BADSHAPE),
    ("a sample past an int", dict(mix=(P, P, 2), H=40000, W=40000), BADSHAPE),
    ("K = 5 and more than 65535 samples: the block's own defect first", dict(mix=(P, P, 5), B=70000), BADARG),
]


@pytest.mark.parametrize("what,kw,code", MIX_DEFECTS, ids=[d[0] for d in MIX_DEFECTS])
def test_chain_mix_reports_each_defect(what, kw, code):
    assert _call(**kw) == code


def test_valid_blended_call_reaches_the_workspace_check():
    for K in (1, 2, 3, 4):
        assert _call(mix=(P, P + 4, K)) == WORKSPACE                     # (weights: 4-byte alignment is enough)
    assert _call(mix=(P + 8, P, 3)) == WORKSPACE
    assert _call(mix=(P, P, 2), B=65535) == WORKSPACE
    assert _call(mix=(P, P, 2), B=70000, noise=P) == WORKSPACE           # recorded draws win: the rows are not laid out per sample


def test_block_with_null_keys_changes_nothing():
    """keys = NULL is the call without the block, whatever else the block holds: every case gets the code of
    sinddm_sample_chain_solver."""
    for kw in (dict(), dict(seeds=P), dict(seeds=P + 4), dict(B=70000), dict(seeds=P, B=70000), dict(noise=P + 8)):
        want = _call(entry="sinddm_sample_chain_solver", **kw)
        assert _call(mix="null", **kw) == want, kw
        assert _call(mix=(None, P + 2, 9), **kw) == want, kw
    assert _call(mix=(None, None, 0)) == WORKSPACE


def test_fill_mix_refuses_before_any_device_work():
    lib = _lib.load()
    f = lib.sinddm_normal_fill_mix
    assert f(None, 2, 16, P, P, 2, 0, None) == BADARG
    assert f(P, 2, 16, None, P, 2, 0, None) == BADARG
    assert f(P, 2, 16, P, None, 2, 0, None) == BADARG
    assert f(P, 0, 16, P, P, 2, 0, None) == BADARG
    assert f(P, 2, 0, P, P, 2, 0, None) == BADARG
    assert f(P, 2, 16, P, P, 0, 0, None) == BADARG
    assert f(P, 2, 16, P, P, _lib.MIX_MAX + 1, 0, None) == BADARG
    assert f(P, 2, 16, P + 4, P, 2, 0, None) == BADARG
    assert f(P, 2, 16, P, P + 1, 2, 0, None) == BADARG
    assert f(P, 65536, 16, P, P, 2, 0, None) == BADSHAPE


def test_abi_lists_the_new_symbols():
    assert {"sinddm_sample_chain_mix", "sinddm_normal_fill_mix"} <= set(_lib.ABI_SYMBOLS) and not _lib.missing_symbols()
    assert _lib.load().sinddm_abi_version() == 3


# ---- chain_check itself, under the sanitizers ----------------------------------------------------------------------------------
SAN_MAIN = r"""
#include <cstdio>
#include "chain_run.h"
using namespace sinddm;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
alignas(16) static float dev[64];                               // stands for device memory: only its addresses are used
static sinddm_step_coefs coefs[2];
static int tl[2] = {1, 0};
static ChainRun plain() {
    return chain_run_fill(dev, dev, dev, dev, dev, nullptr, coefs, tl, 2, 0.0f, 1, 0, 160, 4, 8, 12, dev, 0, nullptr, nullptr, nullptr);
}
static int with(const sinddm_mix_opts* mx, ChainChecked* c, void (*more)(ChainRun&) = nullptr) {
    ChainRun r = plain();
    chain_run_set(r, mx);
    if (more) more(r);
    return chain_check(r, c);
}
int main() {
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(dev);
    const uint64_t* keys_off = reinterpret_cast<const uint64_t*>(dev + 1);      // 4 bytes off the 8-byte boundary
    const float* w = dev + 1;                                                    // 4-byte aligned is enough
    const float* w_off = reinterpret_cast<const float*>(reinterpret_cast<const char*>(dev) + 2);
    ChainChecked c;
    // ---- no block, and a block without keys: nothing is set
    CHECK(with(nullptr, &c) == 0 && !c.mkeys && !c.mw && c.mK == 0);
    sinddm_mix_opts none{nullptr, w_off, 9};
    CHECK(with(&none, &c) == 0 && !c.mkeys && !c.mw && c.mK == 0);
    {
        ChainRun r = plain();
        chain_run_set(r, &none);
        CHECK(!r.mix_keys && !r.mix_w && r.mix_K == 0);
    }
    // ---- a valid block, and what the kernels see
    for (int K = 1; K <= SINDDM_MIX_MAX; ++K) {
        sinddm_mix_opts mx{keys, w, K};
        CHECK(with(&mx, &c) == 0 && c.mkeys == reinterpret_cast<const unsigned long long*>(keys) && c.mw == w && c.mK == K && !c.sseeds);
    }
    // ---- every line that refuses, in the function's order
    sinddm_mix_opts k0{keys, w, 0}, k5{keys, w, SINDDM_MIX_MAX + 1}, kneg{keys, w, -1}, now{keys, nullptr, 2}, koff{keys_off, w, 2},
        woff{keys, w_off, 2}, ok{keys, w, 3};
    CHECK(with(&k0, &c) == SINDDM_E_BADARG);
    CHECK(with(&k5, &c) == SINDDM_E_BADARG);
    CHECK(with(&kneg, &c) == SINDDM_E_BADARG);
    CHECK(with(&now, &c) == SINDDM_E_BADARG);
    CHECK(with(&koff, &c) == SINDDM_E_BADARG);
    CHECK(with(&woff, &c) == SINDDM_E_BADARG);
    CHECK(with(&ok, &c, [](ChainRun& r) { r.sample_seeds = reinterpret_cast<const uint64_t*>(dev); }) == SINDDM_E_BADARG);
    CHECK(with(&ok, &c, [](ChainRun& r) { r.B = 65536; }) == SINDDM_E_BADSHAPE);
    CHECK(with(&ok, &c, [](ChainRun& r) { r.B = 65535; }) == 0);
    CHECK(with(&ok, &c, [](ChainRun& r) { r.Hc = r.Wc = 40000; }) == SINDDM_E_BADSHAPE);
    // ---- a refused call resolves nothing
    CHECK(with(&k5, &c) == SINDDM_E_BADARG && !c.mkeys && !c.mw && c.mK == 0);
    // ---- which of two defects is reported
    CHECK(with(&k5, &c, [](ChainRun& r) { r.B = 65536; }) == SINDDM_E_BADARG);                  // the block's own defect first
    CHECK(with(&ok, &c, [](ChainRun& r) { r.halo_y = 3; r.B = 65536; }) == SINDDM_E_BADARG);    // the halo before everything
    CHECK(with(&k5, &c, [](ChainRun& r) { r.x = nullptr; }) == SINDDM_E_BADARG);
    CHECK(with(&ok, &c, [](ChainRun& r) { r.x = nullptr; r.B = 65536; }) == SINDDM_E_BADARG);   // a NULL buffer before the shape
    // ---- recorded draws win over the block: the kernels see no tables, and the per-sample limits do not apply
    CHECK(with(&ok, &c, [](ChainRun& r) { r.noise = dev; }) == 0 && !c.mkeys && !c.mw && c.mK == 0);
    CHECK(with(&ok, &c, [](ChainRun& r) { r.noise = dev; r.B = 65536; }) == 0);
    CHECK(with(&k5, &c, [](ChainRun& r) { r.noise = dev; }) == SINDDM_E_BADARG);               // (the block is still checked)
    // ---- beside every other option
    {
        static float ab[4] = {1, 0, 1, 0};
        static const sinddm_jump_coefs jmp[2] = {{1, 0.5f, 0.5f, 0.0f}, {0, 0, 0, 0}};
        sinddm_chain_opts o{dev, dev, nullptr};
        sinddm_keep_opts k{dev, dev, ab};
        sinddm_resample_opts rs{jmp, nullptr};
        ChainRun r = plain();
        chain_run_set(r, &o); chain_run_set(r, &k); chain_run_set(r, &rs); chain_run_set(r, &ok);
        r.halo_y = 16; r.halo_x = 32;
        CHECK(chain_check(r, &c) == 0 && c.tiled && c.mkeys && c.mK == 3 && c.jumps == jmp && !c.jump_noise);
    }
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails != 0;
}
"""


@pytest.mark.skipif(_host_cxx() is None, reason="no host C++ compiler")
def test_chain_check_with_the_mix_block_under_sanitizers(tmp_path):
    """The same checks on sinddm_amd/csrc/chain_run.h itself: a stand-alone program with its own main, built with the host
    compiler under -fsanitize=address,undefined and run as a plain executable."""
    src, exe = tmp_path / "chain_mix_main.cpp", tmp_path / "chain_mix_main"
    src.write_text(SAN_MAIN)
    subprocess.check_call([_host_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "sinddm_amd", "csrc"), str(src), "-o",
                           str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- the command line and the GIF writer -------------------------------------------------------------------------------------
def test_command_line_builds_the_tables():
    import main
    a = main.parse_args(["--mode", "sample", "--loop_seeds", "1", "2", "3", "--frames", "16", "--gif", "80"])
    assert a.sample_batch_size == 16 and a.seed_mix == loop_seeds(1, 2, 3, 16, 0.5) and a.seeds is None and a.gif == 80
    a = main.parse_args(["--mode", "sample", "--interp_seeds", "4", "5", "--sample_batch_size", "6", "--blend_from_scale", "2"])
    assert a.seed_mix == interp_seeds(4, 5, 6) and a.blend_from_scale == 2
    a = main.parse_args(["--mode", "sample", "--loop_seeds", "1", "2", "3", "--loop_radius", "0.25", "--frames", "4"])
    assert a.seed_mix == loop_seeds(1, 2, 3, 4, 0.25)
    old = main.parse_args(["--mode", "sample", "--seed_base", "3"])       # an old command line: untouched
    assert old.seed_mix is None and old.seeds == [3 + b for b in range(old.sample_batch_size)]
    for argv in (["--interp_seeds", "1", "2", "--loop_seeds", "1", "2", "3"], ["--interp_seeds", "1", "2", "--seed_base", "4"],
                 ["--loop_seeds", "1", "2", "3", "--seeds", "4"], ["--frames", "4"], ["--gif", "80"], ["--blend_from_scale", "1"],
                 ["--loop_seeds", "1", "2", "3", "--loop_radius", "2"], ["--interp_seeds", "1", "2", "--frames", "1"],
                 ["--interp_seeds", "1", "2", "--gif", "0"]):
        with pytest.raises(SystemExit):
            main.parse_args(["--mode", "sample"] + argv)


def test_gif_writer(tmp_path):
    from PIL import Image
    from sinddm_amd.functions import write_gif
    frames = torch.zeros(3, 3, 8, 8)
    frames[0, 0], frames[1, 1], frames[2, 2] = 1.0, 1.0, 1.0              # red, green, blue
    path = write_gif(frames, tmp_path / "loop.gif", 80, loop=0)
    with Image.open(path) as im:
        assert im.n_frames == 3 and im.size == (8, 8) and im.info["loop"] == 0
        seen = []
        for i in range(3):
            im.seek(i)
            assert im.info["duration"] == 80
            seen.append(im.convert("RGB").getpixel((4, 4)))
    assert [max(range(3), key=lambda ch: px[ch]) for px in seen] == [0, 1, 2]          # in order
    once = write_gif(frames, tmp_path / "once.gif", 40, loop=None)
    with Image.open(once) as im:
        assert im.n_frames == 3 and "loop" not in im.info and im.info["duration"] == 40
    with pytest.raises(ValueError):
        write_gif(torch.zeros(3, 8, 8), tmp_path / "bad.gif", 80)
    with pytest.raises(ValueError):
        write_gif(frames, tmp_path / "bad.gif", 0)
