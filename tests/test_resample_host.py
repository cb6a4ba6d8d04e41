"""CPU: RePaint's resampling jumps for known-region sampling -- the schedule (functions.resample_schedule), the exactness of
the jump coefficients on the real C2 tables, the noise-stream layout, the new C-ABI symbols and their argument validation,
the command line and the CLIP refusal.  The GPU side is tests/test_gpu_resample.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from resample_util import closed_form_count, jump_coefs, levels, moment_limits, step_jump_ref, whitened
from sinddm_amd import _lib
from sinddm_amd.configs import CONFIGS, build_diffusion
from sinddm_amd.functions import resample_schedule
from sinddm_amd.models import noise_stream_id

RJ = [(2, 1), (3, 2), (2, 5), (4, 10)]


def _check_walk(t_seq, R, J):
    """The properties of a resampled walk; returns (steps, jump_to)."""
    t_seq = list(t_seq)
    steps, jump_to = resample_schedule(t_seq, R, J)
    assert len(steps) == len(jump_to) == closed_form_count(t_seq, R, J)
    L = t_seq[0]
    level = L                                               # the level the state is at
    for t, l2 in zip(steps, jump_to):
        assert t == level, (t, level)                       # a step never follows a level it does not take as input
        assert t in t_seq
        level = t - 1
        if l2 is not None:
            assert level >= 0 and level % J == 0 and l2 == level + J and l2 <= L
            level = l2
    assert steps[-1] == t_seq[-1] and jump_to[-1] is None
    assert level == t_seq[-1] - 1                           # the walk ends where the plain run ends
    counts = {}
    for t, l2 in zip(steps, jump_to):
        if l2 is not None:
            counts[t - 1] = counts.get(t - 1, 0) + 1
    assert all(c == R - 1 for c in counts.values())
    return steps, jump_to


# ---- 1: the schedule ---------------------------------------------------------------------------------------------------------
def test_worked_example_literally():
    steps, jump_to = resample_schedule(range(9, -1, -1), 2, 3)
    assert steps == [9, 8, 7, 9, 8, 7, 6, 5, 4, 6, 5, 4, 3, 2, 1, 3, 2, 1, 0]
    assert len(steps) == 19
    assert [(i, l) for i, l in enumerate(jump_to) if l is not None] == [(2, 9), (8, 6), (14, 3)]


def test_resample_one_is_the_identity():
    for seq in (list(range(9, -1, -1)), [700, 2, 0], [], [5]):
        for J in (1, 3):
            assert resample_schedule(seq, 1, J) == (list(seq), [None] * len(seq))
    assert resample_schedule(iter([3, 2, 1, 0]), 1, 1)[0] == [3, 2, 1, 0]


@pytest.mark.parametrize("R,J", RJ)
@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_walk_properties_on_every_run_of_c1_and_c2(cfg, R, J):
    ideal = CONFIGS[cfg]["num_timesteps_ideal"]
    runs = [range(ideal[0] - 1, -1, -1)] + [range(n - 2, -1, -1) for n in ideal[1:]]        # p_sample_loop / via_scale_loop
    for i, run in enumerate(runs):
        _check_walk(run, R, J)
    # sample_limited_t: a scale's run stops at the next scale's ideal count instead of 0
    for s in range(len(ideal) - 1):
        top = (ideal[0] if s == 0 else ideal[s] - 1)
        run = list(reversed(range(ideal[s + 1], top)))
        if run:
            steps, _ = _check_walk(run, R, J)
            assert min(steps) == ideal[s + 1]


def test_no_anchors_and_bad_arguments():
    seq = list(range(4, -1, -1))
    assert resample_schedule(seq, 3, 10) == (seq, [None] * 5)            # J > L: no anchor fits below the input level
    assert resample_schedule(seq, 3, 5) == (seq, [None] * 5)             # l + J <= L fails for every multiple of 5
    steps, jump_to = resample_schedule(seq, 2, 4)                        # exactly one anchor: level 0
    assert steps == [4, 3, 2, 1, 4, 3, 2, 1, 0] and jump_to[3] == 4
    _check_walk(range(30, 11, -1), 3, 4)                                 # a run that does not end at 0
    for bad in ((0, 1), (1, 0), (-1, 2)):
        with pytest.raises(ValueError):
            resample_schedule(seq, *bad)
    with pytest.raises(ValueError):
        resample_schedule([9, 7, 5], 2, 2)                               # not a descending run


# ---- 2: exactness of the coefficients ----------------------------------------------------------------------------------------
def test_jump_coefficients_are_exact_on_the_c2_tables():
    """For every (l, l2) the schedules produce on C2, in float64: the jump maps the level-l mean onto the level-l2 mean and the
    level-l variance onto the level-l2 variance, to 1e-12."""
    net, d = build_diffusion("C2", dim=16, device="cpu")
    ideal = d.num_timesteps_ideal
    rng = np.random.default_rng(5)
    worst_m = worst_v = 0.0
    n_pairs = 0
    for s in range(d.n_scales):
        jt = d._jump_table(s)
        sa, sb, g = d._jump_levels(s)
        sa_u, sb_u, g_u = levels(d, s)                      # the restatement's own tables
        assert np.array_equal(sa, sa_u) and np.array_equal(sb, sb_u) and np.array_equal(g, g_u)
        assert (g == 0).all() if s == 0 else (g.max() <= 0.5500001 and g.min() >= 0 and g.max() > 0)
        run = range(ideal[0] - 1, -1, -1) if s == 0 else range(ideal[s] - 2, -1, -1)
        pairs = set()
        for R, J in RJ:
            steps, jump_to = resample_schedule(run, R, J)
            pairs |= {(t - 1, l2) for t, l2 in zip(steps, jump_to) if l2 is not None}
        assert pairs
        for l, l2 in sorted(pairs):
            r, sj, dj = jt(l, l2)
            assert (r, sj, dj) == jump_coefs(d, s, l, l2)
            assert 0.0 < r <= 1.0 and sj >= 0.0 and (s > 0 or dj == 0.0)
            xt, x0 = rng.uniform(-1, 1), rng.uniform(-1, 1)
            M = lambda lv: g[lv] * xt + (1.0 - g[lv]) * x0
            worst_m = max(worst_m, abs(r * sa[l] * M(l) + dj * (xt - x0) - sa[l2] * M(l2)))
            worst_v = max(worst_v, abs(r * r * sb[l] ** 2 + sj * sj - sb[l2] ** 2))
            n_pairs += 1
    print(f"C2, {n_pairs} (l, l2) pairs: worst mean residual {worst_m:.3e}, worst variance residual {worst_v:.3e}")
    assert worst_m <= 1e-12 and worst_v <= 1e-12
    with pytest.raises(ValueError):
        d._jump_table(1)(5, 4)                              # a jump goes up


def test_restatement_keeps_the_marginal_under_a_full_mask():
    """The CPU half of the GPU marginal test: with mask == 1 the step's output is the forward-diffused known image whatever
    the network says, and step + jump (torch.randn in place of Philox) lands on the level-l2 marginal: the whitened residual
    stays inside the five-sigma limits for the N and the levels the GPU test uses.  With z2 = z the variance leaves them."""
    net, d = build_diffusion("C2", dim=16, device="cpu")
    s, B = 1, 2
    H, W = d.image_sizes[s]
    N = B * 3 * H * W
    assert N >= 36000
    gen = torch.Generator().manual_seed(7)
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    k0, xt = (rn(3, H, W) * 0.6).clamp(-1, 1), (rn(B, 3, H, W) * 0.5).clamp(-1, 1)
    lim_m, lim_v = moment_limits(N)
    for t, l2 in ((200, 201), (200, 209), (21, 30)):
        x, eps, z, z2 = rn(B, 3, H, W), rn(B, 3, H, W), rn(B, 3, H, W), rn(B, 3, H, W)
        out = step_jump_ref(d, s, t, l2, x, eps, xt, z, z2, keep=(torch.ones(H, W), k0))
        other = step_jump_ref(d, s, t, l2, x * 0.3, -eps, xt, z, z2, keep=(torch.ones(H, W), k0))
        assert float((out - other).abs().max()) <= 1e-12                 # the network does not matter
        wz = whitened(out, d, s, l2, xt, k0[None].expand(B, -1, -1, -1))
        mean, var = float(wz.mean()), float(wz.var(unbiased=False))
        print(f"t={t} -> level {l2}: N={N} mean {mean:+.4f} (limit {lim_m:.4f}) var {var:.4f} (1 +- {lim_v:.4f})")
        assert abs(mean) <= lim_m and abs(var - 1.0) <= lim_v
        reused = whitened(step_jump_ref(d, s, t, l2, x, eps, xt, z, z, keep=(torch.ones(H, W), k0)), d, s, l2, xt,
                          k0[None].expand(B, -1, -1, -1))
        assert abs(float(reused.var(unbiased=False)) - 1.0) > lim_v      # a reused draw is caught


# ---- 3: host plumbing --------------------------------------------------------------------------------------------------------
def test_jump_stream_ids_are_disjoint_from_every_other_draw():
    assert _lib.JUMP_STREAM == 1 << 31
    top = (1 << 31) - 3                                     # the largest position i < 2^31 - 2
    for s in (0, 1, 5, (1 << 31) - 1):
        lo, hi = noise_stream_id(s, "jump", 0), noise_stream_id(s, "jump", top)
        assert lo == (s << 32) | ((1 << 31) + 2) and hi == (s << 32) | ((1 << 32) - 1)
        # ids are (s << 32) | k and k is monotone in i for both kinds: the two ranges of k do not meet
        assert noise_stream_id(s, "step", top) & 0xffffffff == (1 << 31) - 1 < lo & 0xffffffff
        assert noise_stream_id(s, "init") < noise_stream_id(s, "renoise") < noise_stream_id(s, "step", 0) < lo
        for i in (0, 1, 17, top):
            assert noise_stream_id(s, "jump", i) == noise_stream_id(s, "step", i) + _lib.JUMP_STREAM
            assert noise_stream_id(s, "jump", i) >> 32 == s
    with pytest.raises(ValueError):
        noise_stream_id(0, "jump", top + 1)
    with pytest.raises(ValueError):
        noise_stream_id(0, "jump", -1)


def test_new_symbols_declared_bound_and_structs_mirror():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    lib = _lib.load()
    for name in ("sinddm_sample_chain_resample", "sinddm_reverse_step_jump"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"typedef struct sinddm_jump_coefs \{\s*int on;.*?float r, s, d;\s*\} sinddm_jump_coefs;", txt, re.S)
    assert [f[0] for f in _lib.JumpCoefs._fields_] == ["on", "r", "s", "d"] and C.sizeof(_lib.JumpCoefs) == 16
    m = re.search(r"typedef struct sinddm_resample_opts \{(.*?)\} sinddm_resample_opts;", txt, re.S)
    assert m and re.findall(r"\*\s*(\w+);", m.group(1)) == [f[0] for f in _lib.ResampleOpts._fields_] == ["jumps", "noise"]
    assert C.sizeof(_lib.ResampleOpts) == 2 * C.sizeof(C.c_void_p)
    assert int(re.search(r"#define SINDDM_JUMP_STREAM (0x[0-9a-fA-F]+)ull", txt).group(1), 16) == _lib.JUMP_STREAM
    # the chain entry is sinddm_sample_chain_seeds' signature plus the trailing options
    seeds, rs = lib.sinddm_sample_chain_seeds.argtypes, lib.sinddm_sample_chain_resample.argtypes
    assert list(rs[:-1]) == list(seeds) and rs[-1] is C.POINTER(_lib.ResampleOpts)
    # symbols were added, nothing else
    assert int(re.search(r"#define SINDDM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 3
    assert lib.sinddm_abi_version() == 3
    assert C.sizeof(_lib.StepCoefs) == 13 * 4 and C.sizeof(_lib.KeepOpts) == 3 * C.sizeof(C.c_void_p)
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "missing_symbols" in entry and "_lib.ABI_VERSION" in entry   # build() checks the library against ABI_SYMBOLS
    assert not _lib.missing_symbols()


def test_resample_argument_validation_before_any_device_work():
    lib = _lib.load()
    flag = C.c_int(7)
    tl = (C.c_int * 2)(5, 4)

    def coefs(*modes):
        arr = (_lib.StepCoefs * len(modes))()
        for k, m in zip(arr, modes):
            k.mode = m
        return arr

    def chain(jumps, modes=(0, 0), noise=None, jnoise=None, rs_null=False, xt=None):
        # (fake non-null device pointers: validation returns before anything is enqueued or dereferenced)
        opts = _lib.ChainOpts()
        opts.noise = noise
        rs = _lib.ResampleOpts()
        arr = (_lib.JumpCoefs * 2)(*jumps)
        rs.jumps, rs.noise = C.cast(arr, C.POINTER(_lib.JumpCoefs)), jnoise
        return lib.sinddm_sample_chain_resample(256, 256, 256, 256, 256, xt, coefs(*modes), tl, 2, 0.0, 1, 0, 160, 1, 8, 8, 256, 0,
                                                None, None, C.byref(flag), C.byref(opts), 0, 0, None, None,
                                                None if rs_null else C.byref(rs))

    J = _lib.JumpCoefs
    off, ok = J(0, 0.0, 0.0, 0.0), J(1, 0.8, 0.6, 0.0)
    assert chain([ok, off]) == -3                          # accepted: the (empty) workspace is what fails next
    assert chain([off, off]) == -3 and chain([off, off], rs_null=True) == -3
    assert chain([J(0, 7.0, -1.0, 3.0), off]) == -3        # entries that are off are not read
    assert chain([ok, off], modes=(2, 0)) == -1            # SINDDM_E_BADARG: a jump after a mode-2 step
    assert chain([J(1, 0.0, 1.0, 0.0), off]) == -1         # r outside (0, 1]
    assert chain([J(1, 1.0001, 0.0, 0.0), off]) == -1
    assert chain([J(1, float("nan"), 0.0, 0.0), off]) == -1
    assert chain([J(1, 1.0, 0.0, 0.0), off]) == -3         # r = 1, s = 0 is a jump by no level
    assert chain([J(1, 0.8, -0.6, 0.0), off]) == -1        # s < 0
    assert chain([J(1, 0.8, 0.6, 0.01), off]) == -1        # d != 0 in mode 0
    assert chain([J(1, 0.8, 0.6, 0.01), off], modes=(1, 1), xt=256) == -3
    assert chain([ok, off], jnoise=264) == -1              # a misaligned rs->noise
    assert chain([ok, off], noise=256) == -1               # opts->noise without rs->noise on a run that has jumps
    assert chain([ok, off], noise=256, jnoise=256) == -3
    assert chain([off, off], noise=256) == -3              # ... no jumps: nothing is missing
    assert flag.value == 7

    one = coefs(0)
    jc = J(1, 0.8, 0.6, 0.0)

    def step(x_t=256, eps=256, z=256, z2=256, out=256, k=one, j=jc, ew=None, ec=None, km=None, kx=None, xt=None, B=1):
        return lib.sinddm_reverse_step_jump(x_t, eps, xt, z, z2, out, k, C.byref(j) if j is not None else None, ew, ec, km, kx,
                                            1.0, 0.0, B, 3, 16, None)

    assert step(x_t=None) == -1 and step(z2=None) == -1 and step(out=None) == -1 and step(j=None) == -1 and step(B=0) == -1
    assert step(ew=256) == -1 and step(ec=256) == -1 and step(km=256) == -1 and step(kx=256) == -1      # half a pair
    assert step(k=coefs(2), xt=256) == -1                  # a jump after a mode-2 step
    assert step(k=coefs(1)) == -1                          # mode 1 needs x-tilde
    assert step(j=J(1, 1.5, 0.0, 0.0)) == -1 and step(j=J(1, 0.8, -0.1, 0.0)) == -1 and step(j=J(1, 0.8, 0.6, 0.1)) == -1


def test_command_line_flags():
    import main
    args = main.parse_args(["--mode", "inpaint"])
    assert (args.resample, args.jump_length) == (1, 1)
    args = main.parse_args(["--mode", "outpaint", "--resample", "3", "--jump_length", "10"])
    assert (args.resample, args.jump_length) == (3, 10)
    for bad in (["--resample", "0"], ["--jump_length", "0"], ["--resample", "-2"]):
        with pytest.raises(SystemExit):
            main.parse_args(["--mode", "inpaint"] + bad)


def test_resample_setting_and_clip_refusal():
    net, d = build_diffusion("C1", dim=16, device="cpu")
    assert d.resample is None and d._resample_cfg() is None
    d.resample = (1, 4)
    assert d._resample_cfg() is None                       # R = 1 is the run without jumps
    d.resample = (3, 4)
    assert d._resample_cfg() == (3, 4)
    for bad in ((0, 1), (2, 0)):
        d.resample = bad
        with pytest.raises(ValueError):
            d._resample_cfg()
    d.resample = (2, 2)
    d.clip_guided_sampling = True
    x = torch.zeros(1, 3, 48, 64)
    with pytest.raises(NotImplementedError):
        d._run_steps(x, 0, [3, 2, 1, 0])
    with pytest.raises(NotImplementedError):
        d._p_sample_host_t(x, 3, 0, jump_to=4)
