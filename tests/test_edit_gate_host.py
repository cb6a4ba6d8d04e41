"""Per-pixel edit strength on the host (no GPU): the level-gated keep of the sampler chain up to the first device call.
  1. functions.gate_thresholds: the rule thr = 1 - (land + 1) / (t_top + 1) in float64 -> fp32 for a plain, a strided and a
     resampled run; the range (0, 1]; 1 exactly on landing clean; strictly increasing over a plain run;
  2. functions.hold_pyramid: constant maps stay constant, {0, 1} maps on block-aligned regions stay {0, 1} and agree with
     keep_mask_pyramid of the inverted map, the batch dimension;
  3. sampler.RunPlan: `Step.thr` iff `keep_gated`, `pack_steps` emits the array, the refusals, the single-step plan with `t_top`;
  4. chain_check: a threshold of 0, above 1, NaN, a gate without maps -- through the library on fake pointers (refused before
     any device work) and in a stand-alone program over chain_run.h;
  5. header, binding and library agree on the two new entries; the gated entry with gt = NULL reports what _mix reports;
  6. main.py: the new mode's flags, per-job expansion, `--mode edit` without `--edit_map`."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from sinddm_amd import _lib
from sinddm_amd.configs import build_diffusion
from sinddm_amd.functions import gate_thresholds, hold_pyramid, keep_mask_pyramid, resample_schedule, stride_schedule
from sinddm_amd.sampler import NOT_BUILT, RunPlan, pack_steps
from test_batch_maps_host import REPO, _host_cxx

B, H, W, T_SEQ = 3, 8, 12, list(range(9, -1, -1))


def _rule(lands, t_top):
    return [float(np.float32(1.0 - (float(u) + 1.0) / (float(t_top) + 1.0))) for u in lands]


# ---- 1: thresholds -------------------------------------------------------------------------------------------------------
def test_gate_thresholds_plain_strided_resampled():
    plain = gate_thresholds([t - 1 for t in T_SEQ], 9)
    assert plain.dtype == np.float32 and plain.tolist() == _rule(range(8, -2, -1), 9)
    assert float(plain[-1]) == 1.0 and float(plain[0]) == float(np.float32(0.1))
    assert bool(np.all(np.diff(plain.astype(np.float64)) > 0))                   # strictly increasing over a plain run
    taus, lands = stride_schedule(list(range(99, -1, -1)), 7)
    strided = gate_thresholds(lands, 99)
    assert strided.tolist() == _rule(lands, 99) and float(strided[-1]) == 1.0 and lands[-1] == -1
    steps, jump_to = resample_schedule(T_SEQ, 2, 3)
    assert len(steps) > len(T_SEQ) and max(steps) == 9                           # (the expansion does not raise the top)
    res = gate_thresholds([t - 1 for t in steps], 9)
    assert res.tolist() == _rule([t - 1 for t in steps], 9)
    # after a jump back up the threshold falls again: a released pixel is pinned until the run is back at its level
    i = next(i for i, j in enumerate(jump_to) if j is not None)
    assert float(res[i + 1]) < float(res[i])
    for thr in (plain, strided, res, gate_thresholds([-1], 0), gate_thresholds([998, 0, -1], 999)):
        assert bool(np.all((thr > 0.0) & (thr <= 1.0)))
    assert gate_thresholds([], 5).shape == (0,)
    for lands, top in (([9], 9), ([-2], 9), ([0], -1)):                           # a land at or above the top, below clean
        with pytest.raises(ValueError):
            gate_thresholds(lands, top)


def test_gate_rule_in_terms_of_strength():
    """h = 1 - strength is kept on landing at u iff strength <= (u + 1) / (t_top + 1): 0 always, 1 never, 0.5 on the upper half."""
    thr = gate_thresholds(list(range(18, -2, -1)), 19).astype(np.float64)        # T = 20: lands 18 .. -1
    kept = lambda strength: [bool(np.float32(1.0 - strength) >= np.float32(v)) for v in thr]
    assert all(kept(0.0)) and not any(kept(1.0))
    assert kept(0.5) == [u + 1 >= 10 for u in range(18, -2, -1)]


# ---- 2: hold pyramids ----------------------------------------------------------------------------------------------------
SIZES = [(5, 7), (9, 13), (16, 24), (32, 48)]


def test_hold_pyramid_constant_binary_and_batch():
    for c in (0.0, 0.25, 0.3, 1.0):
        pyr = hold_pyramid(torch.full((32, 48), c), SIZES)
        assert [tuple(p.shape) for p in pyr] == SIZES and all(p.dtype == torch.float32 for p in pyr)
        for p in pyr:
            assert float(p.min()) == float(p.max()) == float(np.float32(1.0 - c))
    # a {0, 1} map whose regions are whole footprints at the sizes that divide 32 x 48 evenly (16 x 24, and the map's own)
    st = torch.zeros(32, 48)
    st[8:20, 12:40] = 1
    pyr = hold_pyramid(st, SIZES)
    inv = keep_mask_pyramid(1 - st, SIZES, hard=True)
    for p, m, size in zip(pyr, inv, SIZES):
        if size in ((16, 24), (32, 48)):
            assert set(p.unique().tolist()) == {0.0, 1.0} and torch.equal(p, m)
        assert float(p.min()) >= 0.0 and float(p.max()) <= 1.0
    assert torch.equal(pyr[-1], 1 - st)
    # the batch dimension: row b is the call on map b alone
    stack = torch.stack([st, torch.full((32, 48), 0.6), 1 - st])
    rows = hold_pyramid(stack, SIZES, batch=True)
    assert [tuple(r.shape) for r in rows] == [(3,) + s for s in SIZES]
    for b in range(3):
        assert all(torch.equal(r[b], one) for r, one in zip(rows, hold_pyramid(stack[b], SIZES)))
    for bad, kw in ((stack, {}), (st, dict(batch=True)), (st * 2, {}), (st - 0.5, {}), (torch.zeros(4, 4), {})):
        with pytest.raises(ValueError):
            hold_pyramid(bad, SIZES, **kw)


# ---- 3: the run plan -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    net, d = build_diffusion("C2", dim=20, device="cpu")
    d.omega = 0.3
    d.img_prev_upsample = torch.zeros(B, 3, H, W)
    return d


@pytest.fixture
def gated(model):
    saved = {k: getattr(model, k) for k in ("keep_maps", "keep_gated", "resample", "sample_steps", "clip_guided_sampling",
                                            "solver_order")}
    model.keep_maps = {s: (torch.full((H, W), 0.5), torch.zeros(3, H, W)) for s in (0, 1)}
    model.keep_gated = True
    yield model
    for k, v in saved.items():
        setattr(model, k, v)


@pytest.mark.parametrize("s", [0, 1])
def test_run_plan_carries_thresholds_iff_gated(gated, s):
    d, img = gated, torch.zeros(B, 3, H, W)
    plan = RunPlan(d, img, s, T_SEQ)
    assert plan.gated and [st.thr for st in plan.steps] == _rule([st.land for st in plan.steps], 9)
    floats = lambda vals: struct.pack(f"{len(vals)}f", *vals)
    for i0, k in ((0, 10), (2, 5)):
        p = pack_steps(plan, i0, k)
        assert bytes(p.thr) == floats([st.thr for st in plan.steps[i0:i0 + k]]) and len(p.thr) == k
        assert bytes(p.ab) == floats([v for st in plan.steps[i0:i0 + k] for v in st.ab])
    d.keep_gated = False
    plain = RunPlan(d, img, s, T_SEQ)
    assert not plain.gated and all(st.thr is None for st in plain.steps) and pack_steps(plain, 0, 10).thr is None
    # everything else of a record does not depend on the gate
    other = lambda st: (st.pos, st.t, st.land, bytes(st.k), st.ab, st.jump_to, st.g, st.q)
    assert [other(a) for a in plan.steps] == [other(b) for b in plain.steps]
    d.keep_gated = True
    # strided and resampled runs: the rule reads Step.land; the top is that of the run as handed over
    d.sample_steps = 4
    few = RunPlan(d, img, s, T_SEQ)
    assert len(few.steps) == 4 and [st.thr for st in few.steps] == _rule([st.land for st in few.steps], 9)
    d.sample_steps, d.resample = None, (2, 3)
    res = RunPlan(d, img, s, T_SEQ)
    assert len(res.steps) > 10 and [st.thr for st in res.steps] == _rule([st.t - 1 for st in res.steps], 9)
    d.resample = None
    # the single-step plan with t_top holds the run's own record
    for st in plan.steps:
        one = RunPlan(d, img, s, [st.t], at=(st.pos, None, None, None, 9))
        assert len(one.steps) == 1 and one.steps[0].thr == st.thr and bytes(one.steps[0].k) == bytes(st.k)
    with pytest.raises(_lib.SinddmError, match="no CPU fallback"):           # (the route stops at the network: no GPU here)
        d._p_sample_host_t(img, 5, s, t_top=9)
    assert RunPlan(d, img, s, []).steps == []


def test_run_plan_refusals(gated):
    d, img = gated, torch.zeros(B, 3, H, W)
    with pytest.raises(ValueError, match="t_top"):
        RunPlan(d, img, 1, [5], at=(0, None, None, None))                    # a gated single step without its run's top
    with pytest.raises(ValueError, match="t_top"):
        d._p_sample_host_t(img, 5, 1)
    d.keep_maps = {0: d.keep_maps[0]}
    with pytest.raises(ValueError, match="keep_gated without keep_maps"):
        RunPlan(d, img, 1, T_SEQ)                                            # no entry for the scale
    d.keep_maps = None
    with pytest.raises(ValueError, match="keep_gated without keep_maps"):
        RunPlan(d, img, 1, T_SEQ)
    d.keep_maps = {1: (torch.ones(H, W), torch.zeros(3, H, W))}
    d.clip_guided_sampling = True
    with pytest.raises(NotImplementedError) as err:
        RunPlan(d, img, 1, T_SEQ)
    assert str(err.value) in NOT_BUILT.values() and ("keep_gated", "clip") in NOT_BUILT
    d.keep_gated = False
    with pytest.raises(NotImplementedError) as err:
        RunPlan(d, img, 1, T_SEQ)
    assert str(err.value) == NOT_BUILT["keep_maps", "clip"]


# ---- 4, 5: the C ABI -----------------------------------------------------------------------------------------------------
BADARG, WORKSPACE = -1, -3
P = 4096                                                                     # a fake device pointer, 16-byte aligned


def _gate_call(thr, keep=True, gate=True, entry="sinddm_sample_chain_gate"):
    """The entry on fake pointers and an empty workspace: a valid call ends at SINDDM_E_WORKSPACE, nothing is enqueued."""
    lib = _lib.load()
    coefs = (_lib.StepCoefs * 2)()
    tl = (C.c_int * 2)(1, 0)
    flag = C.c_int(7)
    ab = (C.c_float * 4)(1.0, 0.0, 1.0, 0.0)
    kopts = _lib.KeepOpts(P, P, C.cast(ab, C.POINTER(C.c_float))) if keep else None
    arr = (C.c_float * 2)(*thr) if thr is not None else None
    gopts = _lib.GateOpts(C.cast(arr, C.POINTER(C.c_float)) if arr is not None else None)
    ref = lambda o: C.byref(o) if o is not None else None
    args = [P, P, P, P, P, P, coefs, tl, 2, 0.0, 1, 0, 160, 4, 8, 8, P, 0, None, None, C.byref(flag), None, 0, 0, ref(kopts), None,
            None, None, None, None, None]
    if entry == "sinddm_sample_chain_gate":
        args.append(ref(gopts) if gate else None)
    rc = getattr(lib, entry)(*args)
    assert flag.value == 7
    return rc


def test_chain_check_refuses_a_bad_gate_before_device_work():
    assert _gate_call([0.2, 1.0]) == WORKSPACE                               # a valid gate: every check passed
    assert _gate_call([1.0, 1.0]) == WORKSPACE and _gate_call([1e-30, 0.5]) == WORKSPACE
    for bad in ([0.0, 0.5], [0.5, 0.0], [-0.25, 0.5], [0.5, 1.0000001], [2.0, 0.5], [float("nan"), 0.5], [0.5, float("inf")]):
        assert _gate_call(bad) == BADARG, bad
    assert _gate_call([0.5, 0.5], keep=False) == BADARG                      # a gate without keep maps
    # gt = NULL and gt->thr = NULL are sinddm_sample_chain_mix: the same verdicts
    for keep in (True, False):
        want = _gate_call(None, keep=keep, entry="sinddm_sample_chain_mix")
        assert want == WORKSPACE
        assert _gate_call(None, keep=keep) == want and _gate_call(None, keep=keep, gate=False) == want


def test_reverse_step_keep_gate_arguments():
    lib = _lib.load()
    k = _lib.StepCoefs()
    call = lambda thr, km=P, n=4: lib.sinddm_reverse_step_keep_gate(P, P, None, P, P, C.byref(k), None, None, km, P, 1.0, 0.0, n, 3,
                                                                    16, None, thr)
    for thr in (0.0, -1.0, 1.5, float("nan")):
        assert call(thr) == BADARG
    assert call(0.5, km=None) == BADARG and call(0.5, n=0) == BADARG          # what sinddm_reverse_step_keep refuses


def test_header_binding_and_library_agree_on_the_gate():
    with open(os.path.join(REPO, "include", "sinddm_hip.h")) as f:
        txt = f.read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("sinddm_sample_chain_gate", "sinddm_reverse_step_keep_gate"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code) and name in _lib.ABI_SYMBOLS and hasattr(_lib.load(), name)
    assert re.search(r"typedef struct sinddm_gate_opts\s*\{\s*const float\*\s*thr;\s*\}\s*sinddm_gate_opts;", code)
    assert [f[0] for f in _lib.GateOpts._fields_] == ["thr"] and C.sizeof(_lib.GateOpts) == C.sizeof(C.c_void_p)
    lib = _lib.load()
    assert lib.sinddm_sample_chain_gate.argtypes[:-1] == lib.sinddm_sample_chain_mix.argtypes
    assert lib.sinddm_reverse_step_keep_gate.argtypes[:-1] == lib.sinddm_reverse_step_keep.argtypes
    assert lib.sinddm_abi_version() == _lib.ABI_VERSION == 3
    assert not _lib.missing_symbols()
    # the contract the header states
    block = txt[txt.index("per-pixel edit strength"):txt.index("int sinddm_sample_chain_gate")]
    for phrase in (">= thr[i]", "fp32 compare", "switches the soft blend off", "binary mask makes the gate invisible", "sigma != 0 or keep_b != 0"):
        assert phrase in block, phrase


GATE_MAIN = r"""
#include <cmath>
#include <cstdio>
#include "chain_run.h"
using namespace sinddm;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
alignas(16) static float dev[64];
static sinddm_step_coefs coefs[3];
static int tl[3] = {2, 1, 0};
static float ab[6] = {1, 0, 1, 0, 1, 0};
static int check(const float* thr, bool keep, int n = 3) {
    ChainRun r = chain_run_fill(dev, dev, dev, dev, dev, dev, coefs, tl, n, 0.0f, 1, 0, 160, 4, 8, 12, dev, 0, nullptr, nullptr, nullptr);
    sinddm_keep_opts k{dev, dev, ab};
    sinddm_gate_opts g{thr};
    if (keep) chain_run_set(r, &k);
    chain_run_set(r, &g);
    ChainChecked c;
    return chain_check(r, &c);
}
int main() {
    static const float ok[3] = {0.2f, 0.5f, 1.0f}, zero[3] = {0.2f, 0.0f, 1.0f}, above[3] = {0.2f, 0.5f, 1.5f}, neg[3] = {-0.5f, 0.5f, 1.0f};
    static const float nan_[3] = {0.2f, NAN, 1.0f}, tail[3] = {0.2f, 0.5f, 7.0f};
    CHECK(check(ok, true) == 0);
    CHECK(check(nullptr, true) == 0 && check(nullptr, false) == 0);          // no block: the call without it
    CHECK(check(zero, true) == SINDDM_E_BADARG);
    CHECK(check(above, true) == SINDDM_E_BADARG);
    CHECK(check(neg, true) == SINDDM_E_BADARG);
    CHECK(check(nan_, true) == SINDDM_E_BADARG);
    CHECK(check(ok, false) == SINDDM_E_BADARG);                               // a gate without keep maps
    CHECK(check(tail, true, 2) == 0);                                         // only n_steps entries are read
    CHECK(gate_valid(1.0f) && gate_valid(1e-30f) && !gate_valid(0.0f) && !gate_valid(-0.0f) && !gate_valid(INFINITY));
    ChainRun r{};
    chain_run_set(r, static_cast<const sinddm_gate_opts*>(nullptr));
    CHECK(r.gate_thr == nullptr);
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails != 0;
}
"""


@pytest.mark.skipif(_host_cxx() is None, reason="no host C++ compiler")
def test_gate_check_stand_alone(tmp_path):
    """chain_run.h stays free of HIP: a plain C++ program with its own main includes it and walks the gate's lines, under
    -fsanitize=address,undefined like the chain-options program beside it."""
    src, exe = tmp_path / "gate_main.cpp", tmp_path / "gate_main"
    src.write_text(GATE_MAIN)
    subprocess.check_call([_host_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "sinddm_amd", "csrc"), str(src), "-o",
                           str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 6: the command line -------------------------------------------------------------------------------------------------
def test_main_edit_flags(capsys):
    import main
    a = main.parse_args(["--mode", "edit", "--edit_map", "m.png"])
    assert a.mode == "edit" and a.edit_map == "m.png" and a.edit_image is None and not isinstance(a.edit_map, main.Jobs)
    assert main.job_values(a.edit_map, 4) == "m.png"
    a = main.parse_args(["--mode", "edit", "--edit_map", "a.png", "b.png", "--edit_image", "x.png", "y.png", "--sample_batch_size",
                         "4", "--seed_base", "3", "--tile", "x", "--resample", "2", "--jump_length", "3", "--sample_steps", "8"])
    assert isinstance(a.edit_map, main.Jobs) and isinstance(a.edit_image, main.Jobs)
    assert main.job_values(a.edit_map, 4) == ["a.png", "b.png", "a.png", "b.png"]
    assert main.job_values(a.edit_image, 4) == ["x.png", "y.png", "x.png", "y.png"]
    assert a.seeds == [3, 4, 5, 6] and a.tile == "x" and (a.resample, a.jump_length) == (2, 3) and a.sample_steps == [8]
    assert "edit_map" in main._PER_JOB and "edit_image" in main._PER_JOB
    with pytest.raises(SystemExit):
        main.parse_args(["--mode", "edit", "--edit_map", "a.png", "b.png", "c.png", "--sample_batch_size", "4"])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        main.parse_args(["--mode", "edit"])
    assert e.value.code != 0 and "--mode edit needs --edit_map" in capsys.readouterr().err
    assert main.parse_args(["--mode", "sample"]).edit_map is None              # the other modes do not ask for it
    assert "--edit_map" in main.__doc__ and "--edit_image" in main.__doc__
