"""CPU: the interface of the fused sampler chain with options (sinddm_sample_chain_ex: ROI edit maps and caller-supplied
noise) -- header, ctypes binding, argument validation and the Python switches that route a run onto it."""
import ctypes as C
import os
import re

from conftest import REPO
from sinddm_amd import _lib
from sinddm_amd.models import MultiScaleGaussianDiffusion, SinDDMNet


def test_chain_ex_declared_bound_and_opts_mirror():
    txt = open(os.path.join(REPO, "include", "sinddm_hip.h")).read()
    assert re.search(r"\bint\s+sinddm_sample_chain_ex\s*\(", txt)
    assert "sinddm_sample_chain_ex" in _lib.ABI_SYMBOLS
    m = re.search(r"typedef struct sinddm_chain_opts \{(.*?)\} sinddm_chain_opts;", txt, re.S)
    assert m, "struct sinddm_chain_opts is not in the header"
    fields = re.findall(r"const float\*\s*(\w+);", m.group(1))
    assert fields == [f[0] for f in _lib.ChainOpts._fields_] == ["edit_w", "edit_c", "noise"]
    assert C.sizeof(_lib.ChainOpts) == 3 * C.sizeof(C.c_void_p)
    assert int(re.search(r"#define SINDDM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 3   # a symbol was added, no more
    assert hasattr(_lib.load(), "sinddm_sample_chain_ex")


def test_chain_ex_rejects_half_an_edit_before_any_device_work():
    lib = _lib.load()
    one = C.cast(C.pointer(_lib.StepCoefs()), C.POINTER(_lib.StepCoefs))
    tl = (C.c_int * 1)(0)
    flag = C.c_int(7)

    def call(opts, n_steps=1):
        # (fake non-null device pointers: validation returns before anything is enqueued or dereferenced)
        return lib.sinddm_sample_chain_ex(256, 256, 256, 256, 256, None, one, tl, n_steps, 0.0, 1, 0, 160, 1, 8, 8, 256, 0, None,
                                          None, C.byref(flag), C.byref(opts) if opts is not None else None)

    o = _lib.ChainOpts()
    o.edit_w = 256
    assert call(o) == -1                                   # SINDDM_E_BADARG: edit_w without edit_c
    o = _lib.ChainOpts()
    o.edit_c = 256
    assert call(o) == -1
    o = _lib.ChainOpts()
    o.edit_w, o.edit_c, o.noise = 256, 256, 260            # not 16-byte aligned
    assert call(o) == -1
    o.noise = 256
    assert call(o) == -3                                   # arguments accepted: the (empty) workspace is what fails next
    assert call(None) == -3
    assert flag.value == 7


def test_chain_switches_default_to_the_pinned_routes():
    net = SinDDMNet(dim=16, multiscale=True, device="cpu")
    d = MultiScaleGaussianDiffusion(net, n_scales=3, scale_factor=1.4, image_sizes=[(64, 48), (90, 67), (126, 94)],
                                    timesteps=20, train_full_t=True, scale_losses=[1.08, 0.77], loss_factor=1, loss_type="l1",
                                    device="cpu")
    assert d.chain_noise is False          # a noise_fn keeps the step-by-step path unless asked otherwise
    assert d.chain_guided is True          # ROI guidance rides the chain call
    from sinddm_amd import models
    assert 4 * 161_000_000 <= models.CHAIN_NOISE_BYTES      # C3's finest scale at batch 64: several steps per call
