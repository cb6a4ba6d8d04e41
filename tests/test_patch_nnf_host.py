"""CPU: the host side of the patch nearest-neighbour field -- the two C entries are declared, bound and exported; their
argument checks run before any device work; `metrics.nnf_stats` on hand-made fields; the `evaluate` command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from sinddm_amd import _lib

ENTRIES = ("sinddm_patch_nnf_workspace_bytes", "sinddm_patch_nnf")


def test_entries_are_declared_bound_and_exported():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.sinddm_abi_version() == 3                       # nothing that existed changed


def test_workspace_grows_with_the_reference():
    lib = _lib.load()
    a = lib.sinddm_patch_nnf_workspace_bytes(2, 29, 37, 29, 37, 7, 0, 0)
    b = lib.sinddm_patch_nnf_workspace_bytes(2, 29, 37, 58, 74, 7, 0, 0)
    c = lib.sinddm_patch_nnf_workspace_bytes(2, 29, 37, 29, 37, 7, 0, 3)      # a wrapped reference has more positions
    assert 0 < a < b and a < c
    # at least |b|^2 of every reference position and one 64-bit key per query
    assert a >= 2 * (23 * 31) * 4 + 2 * (23 * 31) * 8
    assert lib.sinddm_patch_nnf_workspace_bytes(2, 29, 37, 29, 37, 4, 0, 0) == 0
    assert lib.sinddm_patch_nnf_workspace_bytes(0, 29, 37, 29, 37, 7, 0, 0) == 0
    assert lib.sinddm_patch_nnf_workspace_bytes(1, 6, 37, 29, 37, 7, 0, 0) == 0


def test_argument_errors_come_before_any_device_work():
    lib = _lib.load()
    buf = (C.c_float * 16)()                                  # never dereferenced: every call below is refused
    p = C.cast(buf, C.c_void_p)
    big = 1 << 30

    def call(query=p, ref=p, dist=p, idx=p, B=1, Hq=29, Wq=37, Hr=29, Wr=37, P=7, ws=p, ws_bytes=big):
        return lib.sinddm_patch_nnf(query, 1, ref, 0, None, dist, idx, B, Hq, Wq, Hr, Wr, P, 0, 0, ws, ws_bytes, None)

    for kw in (dict(query=None), dict(ref=None), dict(dist=None), dict(idx=None), dict(ws=None), dict(B=0), dict(P=4),
               dict(P=9), dict(ws_bytes=16)):
        assert call(**kw) == -1, kw
    assert call(Hq=6) == -2                                   # an axis shorter than the patch
    assert call(Wr=6) == -2
    assert call(Hr=50000, Wr=50000) == -2                     # 2^31 reference positions or more
    assert call(Hq=4, P=5) == -2 and call(Hq=2, P=3) == -2


def _identity(h, w, shift=(0, 0)):
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack([ys + shift[0], xs + shift[1]])[None].to(torch.int32)


def test_nnf_stats_identity_shift_and_shuffle():
    from sinddm_amd.metrics import nnf_stats
    h, w, P = 23, 31, 7
    zero = torch.zeros(1, h, w)
    st = nnf_stats(zero, _identity(h, w), P, (h, w))
    assert float(st["coherence"][0]) == 1.0 and float(st["fidelity"][0]) == 0.0 and "seam" not in st
    st = nnf_stats(zero, _identity(h, w, (3, -2)), P, (h + 8, w + 8))
    assert float(st["coherence"][0]) == 1.0
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(h * w, generator=g)
    yx = torch.stack([perm // w, perm % w]).reshape(1, 2, h, w).to(torch.int32)
    st = nnf_stats(zero, yx, P, (h, w))
    assert float(st["coherence"][0]) < 0.05
    # fidelity is the mean distance per patch element, per sample
    d = torch.rand(2, h, w, generator=g)
    st = nnf_stats(d, _identity(h, w).repeat(2, 1, 1, 1), P, (h, w))
    assert torch.allclose(st["fidelity"], d.double().mean(dim=(1, 2)) / (3 * P * P), rtol=1e-12, atol=0)
    # one broken position breaks itself, its left and its upper neighbour
    yx = _identity(h, w).clone()
    yx[0, :, 5, 7] = 0
    st = nnf_stats(zero, yx, P, (h, w))
    assert float(st["coherence"][0]) == pytest.approx(1.0 - 3.0 / ((h - 1) * (w - 1)), abs=1e-12)


def test_nnf_stats_seam_counts_the_crossing_positions():
    from sinddm_amd.metrics import nnf_stats
    H, W, P = 12, 15, 5
    ys, xs = np.mgrid[0:H, 0:W]
    for wrap in ((False, True), (True, False), (True, True)):
        cross = np.zeros((H, W), bool)
        if wrap[0]:
            cross |= ys > H - P
        if wrap[1]:
            cross |= xs > W - P
        assert int(cross.sum()) == {(False, True): H * (P - 1), (True, False): W * (P - 1),
                                    (True, True): H * (P - 1) + W * (P - 1) - (P - 1) ** 2}[wrap]
        d = torch.from_numpy(np.where(cross, 6.0, 2.0))[None].float()
        st = nnf_stats(d, _identity(H, W), P, (H, W), wrap_query=wrap)
        assert float(st["seam"][0]) == pytest.approx(3.0, rel=1e-12)
        # one more position on either side of the rule would change the ratio
        d2 = d.clone()
        if wrap[1]:
            d2[0, 0, W - P] = 100.0                           # x == W - P does not cross
        else:
            d2[0, H - P, 0] = 100.0
        st2 = nnf_stats(d2, _identity(H, W), P, (H, W), wrap_query=wrap)
        n_other = H * W - int(cross.sum())
        assert float(st2["seam"][0]) == pytest.approx(6.0 / ((2.0 * (n_other - 1) + 100.0) / n_other), rel=1e-12)
    assert "seam" not in nnf_stats(torch.ones(1, H, W), _identity(H, W), P, (H, W))


def test_nnf_stats_offsets_modulo_a_wrapped_reference():
    from sinddm_amd.metrics import nnf_stats
    h, w, P = 9, 11, 3
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    # a copy shifted by (0, 4) of a reference that wraps in x: the coordinates fold back, the offsets jump by the grid width
    yx = torch.stack([ys, (xs + 4) % w])[None].to(torch.int32)
    zero = torch.zeros(1, h, w)
    assert float(nnf_stats(zero, yx, P, (h, w), wrap_ref=(False, True))["coherence"][0]) == 1.0
    assert float(nnf_stats(zero, yx, P, (h, w), wrap_ref=(False, False))["coherence"][0]) < 1.0
    assert float(nnf_stats(zero, yx, P, (h, w), wrap_ref=(True, False))["coherence"][0]) < 1.0
    # on a wrapped QUERY axis the neighbour across the border counts: the same field, query and reference both wrapped
    st = nnf_stats(zero, yx, P, (h, w), wrap_query=(False, True), wrap_ref=(False, True))
    assert float(st["coherence"][0]) == 1.0


def test_command_line_knows_evaluate():
    import main
    a = main.parse_args(["--mode", "evaluate", "--eval_patch", "5"])
    assert a.mode == "evaluate" and a.eval_patch == 5 and a.eval_scale is None
    a = main.parse_args(["--mode", "evaluate", "--eval_scale", "2", "--tile", "x", "--sample_steps", "4", "--seed_base", "7",
                         "--sample_batch_size", "2"])
    assert a.eval_patch == 7 and a.eval_scale == 2 and a.tile == "x" and a.seeds == [7, 8]
    with pytest.raises(SystemExit):
        main.parse_args(["--mode", "evaluate", "--eval_patch", "4"])
    with pytest.raises(SystemExit):
        main.parse_args(["--mode", "evaluate", "--eval_scale", "-1"])
    assert "evaluate" in open(os.path.join(REPO, "main.py")).read().split("raise NotImplementedError")[0]


def test_cpu_tensors_are_refused():
    from sinddm_amd.metrics import patch_nnf, patch_report
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(_lib.SinddmError, match="no CPU fallback"):
        patch_nnf(x, x, patch=5)
    with pytest.raises(_lib.SinddmError):
        patch_report(x, x[0], patch=5)
