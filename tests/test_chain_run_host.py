"""The sampler chain's host side before any device work (no GPU): every sinddm_sample_chain* entry fills one internal
description (sinddm_amd/csrc/chain_run.h) and runs one body, so an argument set gets the same error code from every entry
whose signature can express it -- through the library with fake pointers -- and the check function itself, line by line,
in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

from sinddm_amd import _lib
from test_batch_maps_host import REPO, _host_cxx

BADARG, BADSHAPE, WORKSPACE = -1, -2, -3
P = 4096                                                                 # a fake device pointer, 16-byte aligned
# the entries by what their signatures can express: each has every option of the ones before it
ENTRIES = ["sinddm_sample_chain", "sinddm_sample_chain2", "sinddm_sample_chain_ex", "sinddm_sample_chain_tile",
           "sinddm_sample_chain_keep", "sinddm_sample_chain_seeds", "sinddm_sample_chain_resample", "sinddm_sample_chain_layout",
           "sinddm_sample_chain_batch"]
NEEDS = {"edit": 2, "noise": 2, "halo": 3, "keep": 4, "seeds": 5, "jumps": 6, "jump_noise": 6, "lay": 7, "batch": 8}


def _call(level, x=P, n=2, dim=160, B=4, H=8, W=8, modes=(0, 0), edit=(None, None), noise=None, halo=(0, 0), keep=None, seeds=None,
          jumps=None, jump_noise=None, lay=None, batch=None):
    """ENTRIES[level] on fake pointers and an empty workspace, or None where its signature cannot say what is asked.  keep =
    (mask, x0, with_ab), jumps = [(on, r, s, d)] * n, lay = (layout, down, g or None, delta), batch = (4 flags, gain)."""
    asked = dict(edit=edit != (None, None), noise=noise, halo=halo != (0, 0), keep=keep, seeds=seeds, jumps=jumps,
                 jump_noise=jump_noise, lay=lay, batch=batch)
    if any(v and level < NEEDS[k] for k, v in asked.items()):
        return None
    lib = _lib.load()
    coefs = (_lib.StepCoefs * 2)()
    coefs[0].mode, coefs[1].mode = modes
    tl = (C.c_int * 2)(1, 0)
    flag = C.c_int(7)
    args = [P, P, x, P, P, P, coefs, tl, n, 0.0, 1, 0, dim, B, H, W, P, 0, None]
    args += [C.byref(flag)] if level == 0 else [None, C.byref(flag)]
    ab = (C.c_float * 4)(1.0, 0.0, 1.0, 0.0)
    jarr = (_lib.JumpCoefs * 2)(*[_lib.JumpCoefs(*j) for j in jumps]) if jumps else None
    garr = (C.c_float * 2)(*lay[2]) if lay and lay[2] else None
    blocks = [_lib.ChainOpts(edit[0], edit[1], noise),
              _lib.KeepOpts(keep[0], keep[1], C.cast(ab, C.POINTER(C.c_float)) if keep[2] else None) if keep else None,
              _lib.ResampleOpts(jarr, jump_noise) if jumps or jump_noise else None,
              _lib.LayoutOpts(lay[0], lay[1], garr, lay[3]) if lay else None,
              _lib.BatchOpts(*batch[0], batch[1]) if batch else None]
    ref = lambda o: C.byref(o) if o is not None else None
    tail = [ref(blocks[0]), halo[0], halo[1], ref(blocks[1]), seeds, ref(blocks[2]), ref(blocks[3]), ref(blocks[4])]
    args += tail[:{0: 0, 1: 0, 2: 1, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8}[level]]
    rc = getattr(lib, ENTRIES[level])(*args)
    assert flag.value == 7                                               # nothing was run
    return rc


KEEP, LAY = (P, P, True), (P, 4, (1.0, 0.5), P)
JUMP = [(1, 0.5, 0.5, 0.0), (0, 0.0, 0.0, 0.0)]
DEFECTS = [                                                              # (what, the call, the code every entry returns)
    ("x NULL", dict(x=None), BADARG),
    ("n_steps < 0", dict(n=-1), BADARG),
    ("B = 0", dict(B=0), BADARG),
    ("no such width", dict(dim=7), BADSHAPE),
    ("edit_w without edit_c", dict(edit=(P, None)), BADARG),
    ("edit_c off 16 bytes", dict(edit=(P, P + 4)), BADARG),
    ("noise off 16 bytes", dict(noise=P + 8), BADARG),
    ("edit maps indexed past an int", dict(edit=(P, P), H=40000, W=40000), BADSHAPE),
    ("a halo below the receptive radius", dict(halo=(3, 0)), BADARG),
    ("a halo past 2^20", dict(halo=(0, (1 << 20) + 1)), BADARG),
    ("a halo defect and a NULL buffer", dict(halo=(3, 0), x=None), BADARG),
    ("mask without x0", dict(keep=(P, None, True)), BADARG),
    ("keep maps without ab", dict(keep=(P, P, False)), BADARG),
    ("keep mask off 16 bytes", dict(keep=(P + 4, P, True)), BADARG),
    ("unpaired edit maps and a misaligned keep map", dict(edit=(P, None), keep=(P + 4, P, True)), BADARG),
    ("unpaired edit maps past an int: the pair is checked first", dict(edit=(P, None), H=40000, W=40000), BADARG),
    ("misaligned keep map past an int: the shape is checked first", dict(keep=(P + 4, P, True), H=40000, W=40000), BADSHAPE),
    ("seeds off 8 bytes", dict(seeds=P + 4), BADARG),
    ("seeds for more than 65535 samples", dict(seeds=P, B=70000), BADSHAPE),
    ("a jump on a mode-2 step", dict(jumps=JUMP, modes=(2, 0)), BADARG),
    ("a jump with r > 1", dict(jumps=[(1, 1.5, 0.0, 0.0), (0, 0.0, 0.0, 0.0)]), BADARG),
    ("a jump with d != 0 in mode 0", dict(jumps=[(1, 0.5, 0.5, 0.1), (0, 0.0, 0.0, 0.0)]), BADARG),
    ("jump noise off 16 bytes", dict(jumps=JUMP, jump_noise=P + 4), BADARG),
    ("recorded noise without the jumps' on a run with jumps", dict(jumps=JUMP, noise=P), BADARG),
    ("layout without g", dict(lay=(P, 4, None, P)), BADARG),
    ("g outside [0, 1]", dict(lay=(P, 4, (1.5, 0.0), P)), BADARG),
    ("a jump on a mode-2 step and g out of range", dict(jumps=JUMP, modes=(2, 0), lay=(P, 4, (1.5, 0.0), P)), BADARG),
    ("pull and jump on one step", dict(jumps=JUMP, lay=LAY), BADARG),
    ("down = 0", dict(lay=(P, 0, (1.0, 0.5), P)), BADARG),
    ("no delta scratch", dict(lay=(P, 4, (1.0, 0.5), None)), BADARG),
    ("layout off 16 bytes", dict(lay=(P + 4, 4, (1.0, 0.5), P)), BADARG),
    ("a pull indexed past an int", dict(lay=LAY, H=40000, W=40000), BADSHAPE),
    ("a pull with 3 B planes past 65535", dict(lay=LAY, B=30000), BADSHAPE),
    ("a pull with block rows past 65535", dict(lay=(P, 1, (1.0, 0.5), P), H=70000, W=4), BADSHAPE),
    ("a per-sample flag without its map", dict(batch=((0, 1, 0, 0), None)), BADARG),
    ("layout_gain without a layout", dict(batch=((0, 0, 0, 0), P)), BADARG),
    ("no such width and a per-sample flag without its map: the plan comes first", dict(dim=7, batch=((1, 0, 0, 0), None)), BADSHAPE),
]
VALID = [dict(), dict(edit=(P, P), noise=P), dict(halo=(16, 32)), dict(keep=KEEP), dict(seeds=P + 8),
         dict(jumps=JUMP, jump_noise=P, noise=P), dict(lay=LAY), dict(lay=(P + 4, 0, (0.0, 0.0), None)),
         dict(edit=(P, P), noise=P, halo=(16, 16), keep=KEEP, seeds=P, lay=LAY, batch=((1, 1, 1, 1), P),
              jumps=[(0, 9.0, -1.0, 0.0)] * 2, jump_noise=P)]


@pytest.mark.parametrize("what,kw,code", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_every_entry_reports_a_defect_alike(what, kw, code):
    got = {ENTRIES[lv]: _call(lv, **kw) for lv in range(len(ENTRIES))}
    said = {name: rc for name, rc in got.items() if rc is not None}
    assert "sinddm_sample_chain_batch" in said and all(rc == code for rc in said.values()), said
    assert len(said) == len(ENTRIES) - max([NEEDS[k] for k in kw if k in NEEDS], default=0)      # (narrower entries cannot say it)


def test_every_entry_reports_the_workspace_last():
    """An otherwise valid call with ws_bytes = 0: SINDDM_E_WORKSPACE from all nine entries, with each set of options an entry
    can express -- the checks passed, and nothing was enqueued."""
    for kw in VALID:
        got = [_call(lv, **kw) for lv in range(len(ENTRIES))]
        assert got[-1] == WORKSPACE and all(rc in (None, WORKSPACE) for rc in got), (kw, got)
    assert [_call(lv) for lv in range(len(ENTRIES))] == [WORKSPACE] * len(ENTRIES)


SAN_MAIN = r"""
#include <cstdio>
#include "chain_run.h"
using namespace sinddm;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
alignas(16) static float dev[64];                               // stands for device memory: only its addresses are used
static sinddm_step_coefs coefs[3];                              // modes 1, 1, 2: the end of a scale's walk
static int tl[3] = {2, 1, 0};
static float ab[6] = {1, 0, 1, 0, 1, 0};
static ChainRun plain() {
    coefs[0].mode = coefs[1].mode = 1; coefs[2].mode = 2;
    return chain_run_fill(dev, dev, dev, dev, dev, dev, coefs, tl, 3, 0.0f, 1, 0, 160, 4, 8, 12, dev, 0, nullptr, nullptr, nullptr);
}
template <class F> static int with(F&& f, ChainChecked* c = nullptr) {
    ChainRun r = plain();
    f(r);
    ChainChecked local;
    return chain_check(r, c ? c : &local);
}
int main() {
    const float* P = dev;
    const float* off4 = dev + 1;                                // 4 bytes off the 16-byte boundary
    const uint64_t* seeds = reinterpret_cast<const uint64_t*>(dev);
    static const sinddm_jump_coefs jmp[3] = {{1, 0.5f, 0.5f, 0.25f}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    static const sinddm_jump_coefs jmp2[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {1, 0.5f, 0.5f, 0.0f}};    // on the mode-2 step
    static const float g[3] = {1.0f, 0.0f, 0.5f}, g_jump[3] = {0.0f, 1.0f, 0.5f}, g_bad[3] = {0.5f, 1.5f, 0.0f}, g_off[3] = {0, 0, 0};
    ChainChecked c;
    // ---- the plain call, and what it resolves
    CHECK(with([](ChainRun&) {}, &c) == 0 && c.H == 8 && c.W == 12 && !c.tiled && !c.sseeds && !c.jumps && !c.jump_noise && !c.lay_g);
    // ---- every line that refuses, in the function's order
    CHECK(with([](ChainRun& r) { r.halo_y = 3; }) == SINDDM_E_BADARG);
    CHECK(with([](ChainRun& r) { r.halo_x = SINDDM_TILE_HALO - 1; }) == SINDDM_E_BADARG);
    CHECK(with([](ChainRun& r) { r.halo_x = (1 << 20) + 1; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.sample_seeds = reinterpret_cast<const uint64_t*>(off4); }) == SINDDM_E_BADARG);
    CHECK(with([](ChainRun& r) { r.x = nullptr; }) == SINDDM_E_BADARG);
    CHECK(with([](ChainRun& r) { r.coefs = nullptr; }) == SINDDM_E_BADARG);
    CHECK(with([](ChainRun& r) { r.n_steps = -1; }) == SINDDM_E_BADARG);
    CHECK(with([](ChainRun& r) { r.B = 0; }) == SINDDM_E_BADARG);
    CHECK(with([](ChainRun& r) { r.Wc = 0; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.edit_w = P; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.keep_x0 = P; r.keep_ab = ab; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.keep_m = r.keep_x0 = P; }) == SINDDM_E_BADARG);                       // maps without ab
    CHECK(with([&](ChainRun& r) { r.edit_w = r.edit_c = P; r.Hc = r.Wc = 40000; }) == SINDDM_E_BADSHAPE);
    CHECK(with([&](ChainRun& r) { r.keep_m = r.keep_x0 = P; r.keep_ab = ab; r.Hc = r.Wc = 40000; }) == SINDDM_E_BADSHAPE);
    CHECK(with([&](ChainRun& r) { r.sample_seeds = seeds; r.Hc = r.Wc = 40000; }) == SINDDM_E_BADSHAPE);
    CHECK(with([&](ChainRun& r) { r.sample_seeds = seeds; r.B = 65536; }) == SINDDM_E_BADSHAPE);
    CHECK(with([&](ChainRun& r) { r.sample_seeds = seeds; r.B = 65536; r.noise = P; }) == 0);            // recorded draws win: no seeds
    CHECK(with([&](ChainRun& r) { r.edit_w = P; r.edit_c = off4; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.noise = off4; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.keep_m = off4; r.keep_x0 = P; r.keep_ab = ab; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.jumps = jmp2; }) == SINDDM_E_BADARG);
    for (int bad = 0; bad < 4; ++bad) {                          // r = 0, r > 1, s < 0, d without an x-tilde term
        sinddm_jump_coefs j[3] = {{1, bad == 0 ? 0.0f : bad == 1 ? 1.5f : 0.5f, bad == 2 ? -0.1f : 0.5f, 0.0f}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        if (bad == 3) j[0].d = 0.25f;
        CHECK(with([&](ChainRun& r) { r.jumps = j; if (bad == 3) coefs[0].mode = 0; }) == SINDDM_E_BADARG);
    }
    CHECK(with([&](ChainRun& r) { r.jumps = jmp; r.jump_noise = off4; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.jumps = jmp; r.noise = P; }) == SINDDM_E_BADARG);                    // opts->noise without rs->noise
    CHECK(with([&](ChainRun& r) { r.jumps = jmp; r.noise = P; r.jump_noise = P; }, &c) == 0 && c.jumps == jmp && c.jump_noise == P);
    CHECK(with([&](ChainRun& r) { r.jumps = jmp + 1; r.n_steps = 2; r.jump_noise = off4; }, &c) == 0 && !c.jumps && !c.jump_noise);   // none on
    CHECK(with([&](ChainRun& r) { r.layout = P; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g_bad; r.layout_down = 4; r.layout_delta = dev; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 4; r.layout_delta = dev; r.jumps = jmp; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g_jump; r.layout_down = 4; r.layout_delta = dev; r.jumps = jmp; }, &c) == 0 &&
          c.lay_g == g_jump && c.jumps == jmp);                                                            // on different steps
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 0; r.layout_delta = dev; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 65; r.layout_delta = dev; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 4; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.layout = off4; r.layout_g = g; r.layout_down = 4; r.layout_delta = dev; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.layout = off4; r.layout_g = g_off; }, &c) == 0 && !c.lay_g);           // no step pulls: unread
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 4; r.layout_delta = dev; r.Hc = r.Wc = 40000; }) == SINDDM_E_BADSHAPE);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 4; r.layout_delta = dev; r.B = 21846; }) == SINDDM_E_BADSHAPE);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 4; r.layout_delta = dev; r.B = 21845; }) == 0);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 1; r.layout_delta = dev; r.Hc = 65536; r.Wc = 4; }) == SINDDM_E_BADSHAPE);
    CHECK(with([&](ChainRun& r) { r.layout = P; r.layout_g = g; r.layout_down = 2; r.layout_delta = dev; r.Hc = 65536; r.Wc = 4; }) == 0);
    // ---- which of two defects is reported
    CHECK(with([](ChainRun& r) { r.halo_y = 3; r.x = nullptr; }) == SINDDM_E_BADARG);                      // halo defect, NULL buffer
    CHECK(with([&](ChainRun& r) { r.edit_w = P; r.keep_m = off4; r.keep_x0 = P; r.keep_ab = ab; }) == SINDDM_E_BADARG);
    CHECK(with([&](ChainRun& r) { r.edit_w = P; r.Hc = r.Wc = 40000; }) == SINDDM_E_BADARG);               // the pair before the shape
    CHECK(with([&](ChainRun& r) { r.keep_m = off4; r.keep_x0 = P; r.keep_ab = ab; r.Hc = r.Wc = 40000; }) == SINDDM_E_BADSHAPE);   // ... the shape before the alignment
    CHECK(with([&](ChainRun& r) { r.jumps = jmp2; r.layout = P; r.layout_g = g_bad; }) == SINDDM_E_BADARG);   // jump on the mode-2 step, g out of range
    CHECK(with([&](ChainRun& r) { r.x = nullptr; r.edit_w = r.edit_c = P; r.Hc = r.Wc = 40000; }) == SINDDM_E_BADARG);
    // ---- every option on
    sinddm_chain_opts o{P, P, P};
    sinddm_keep_opts k{P, P, ab};
    sinddm_resample_opts rs{jmp, P};
    sinddm_layout_opts lo{P, 4, g_jump, dev};
    sinddm_batch_opts bo{1, 1, 1, 1, P};
    ChainRun r = plain();
    chain_run_set(r, &o); chain_run_set(r, &k); chain_run_set(r, &rs); chain_run_set(r, &lo); chain_run_set(r, &bo);
    r.halo_y = 16; r.halo_x = 32; r.sample_seeds = seeds;
    CHECK(chain_check(r, &c) == 0 && c.tiled && c.H == 8 + 32 && c.W == 12 + 64);
    CHECK(c.sseeds == nullptr && c.jumps == jmp && c.jump_noise == P && c.lay_g == g_jump);                 // (o.noise wins over the seeds)
    CHECK(r.layout_delta == dev && r.layout_down == 4 && r.keep_ab == ab && r.batch.layout_gain == P && r.batch.keep_x0_per_sample == 1);
    o.noise = nullptr;
    r = plain();
    chain_run_set(r, &o); chain_run_set(r, static_cast<const sinddm_keep_opts*>(nullptr)); r.sample_seeds = seeds;
    CHECK(chain_check(r, &c) == 0 && c.sseeds == reinterpret_cast<const unsigned long long*>(seeds) && !r.keep_m && !r.batch.layout_gain);
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails != 0;
}
"""


@pytest.mark.skipif(_host_cxx() is None, reason="no host C++ compiler")
def test_chain_check_under_sanitizers(tmp_path):
    """sinddm_amd/csrc/chain_run.h holds every check of a chain call that needs neither HIP nor the plan: a stand-alone program
    with its own main walks each refusing line, the order of simultaneous defects and a description with every option on,
    under -fsanitize=address,undefined."""
    src, exe = tmp_path / "chain_run_main.cpp", tmp_path / "chain_run_main"
    src.write_text(SAN_MAIN)
    subprocess.check_call([_host_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "sinddm_amd", "csrc"), str(src), "-o",
                           str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
