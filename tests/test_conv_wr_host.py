"""CPU: every refusal of sinddm_debug_conv_wh (include/sinddm_hip_debug.h) happens before a device is touched, and its
scratch size is what the header says: packed binary16 image + per-channel weight scales + per-sample maxima, each rounded
to 256 bytes.  The pointers are made-up addresses: a call that got past its checks would fault, none may."""
import pytest

from sinddm_amd import _lib

BADARG, BADSHAPE = -1, -2
P = 0x10000            # a 256-byte aligned address that is never dereferenced


def _call(lib, variant=2, ncu=0, B=2, H=9, W=36, Wt=0, ci=48, co=160, act=0, x=P, w=P, bias=P, resid=None, aux=None, out=P,
          pre=None, amax=None, scratch=P, nbytes=None):
    if nbytes is None:
        nbytes = 1 << 30
    return lib.sinddm_debug_conv_wh(variant, ncu, B, H, W, Wt, ci, co, act, x, w, bias, resid, aux, out, pre, amax, scratch,
                                    nbytes, None)


def test_scratch_bytes():
    lib = _lib.load()
    f = lib.sinddm_debug_conv_wh_scratch_bytes
    # [co block 2][chunk 3][f 24][n 5][512 halfs] x 2 bytes, 160 floats -> 768, 2 x 8 floats -> 256
    assert f(48, 160, 2) == 2 * 3 * 24 * 5 * 512 * 2 + 768 + 256
    assert f(160, 320, 64) == 4 * 10 * 24 * 5 * 512 * 2 + 1280 + 2048
    assert f(16, 160, 1) == 0 == f(40, 160, 1) == f(48, 100, 1) == f(48, 160, 0) == f(48, 0, 1) == f(48, 160, 65536)


@pytest.mark.parametrize("kw,rc", [
    (dict(x=None), BADARG), (dict(w=None), BADARG), (dict(out=None), BADARG), (dict(scratch=None), BADARG),
    (dict(act=2), BADARG),                                   # GELU' without its pre-activation
    (dict(variant=3), BADARG), (dict(variant=-1), BADARG), (dict(act=3), BADARG),
    (dict(B=0), BADARG), (dict(H=0), BADARG), (dict(W=0), BADARG),
    (dict(W=34), BADSHAPE), (dict(W=37), BADSHAPE),
    (dict(ci=16), BADSHAPE), (dict(ci=40), BADSHAPE), (dict(ci=0), BADARG),
    (dict(co=100), BADSHAPE), (dict(co=40), BADSHAPE),
    (dict(co=240), BADSHAPE), (dict(co=80), BADSHAPE),       # the 160-channel kernel needs whole items
    (dict(Wt=32), BADSHAPE), (dict(Wt=37), BADSHAPE),        # more than three pad columns, wider than the pitch
    (dict(B=65536), BADSHAPE),
    (dict(H=1 << 12, W=1 << 12), BADSHAPE),                  # one sample's input beyond the 32-bit buffer
    (dict(nbytes=0), BADARG), (dict(scratch=P + 16), BADARG),
    (dict(x=P + 4), BADARG), (dict(out=P + 8), BADARG), (dict(resid=P + 4), BADARG), (dict(pre=P + 4), BADARG),
    (dict(act=2, aux=P + 4), BADARG),
])
def test_refusals(kw, rc):
    lib = _lib.load()
    assert _call(lib, **kw) == rc, kw


def test_scratch_one_byte_short():
    lib = _lib.load()
    need = lib.sinddm_debug_conv_wh_scratch_bytes(48, 160, 2)
    assert _call(lib, nbytes=need - 1) == BADARG
    # variants 0 and 1 take Cout = 240; only the size check is left to refuse this call
    assert _call(lib, variant=1, co=240, nbytes=lib.sinddm_debug_conv_wh_scratch_bytes(48, 240, 2) - 1) == BADARG
    assert _call(lib, variant=0, co=240, nbytes=0) == BADARG
