"""Every sinddm_sample_chain* entry fills one description and runs one body: a narrower entry is sinddm_sample_chain_batch with
the same options and NULL for the rest, bit for bit, and `_run_steps` -- which calls sinddm_sample_chain_batch for every run
without multistep factors (sinddm_sample_chain_solver) or a seed blend (sinddm_sample_chain_mix) -- computes what the narrow
entry of each route computes.  dim 20, B = 3, steps [t, 1, 0] with a mode-1 t, on 8x12 (the tail fused into the
network's last kernel: H W % 4 == 0) and 5x7 (unfused: H W % 4 != 0, and dim 20 does not pad its rows; 5x39 under the halo)."""
import ctypes as C

import pytest
import torch

from sinddm_amd import _lib
from sinddm_amd.configs import build_diffusion
from sinddm_amd.models import _workspace, noise_stream_id
from sinddm_amd.synth import hash_randn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S, TS, B, DIM, HALO = 1, [5, 1, 0], 3, 20, _lib.TILE_HALO
ENTRIES = ["", "2", "_ex", "_tile", "_keep", "_seeds", "_resample", "_layout", "_batch"]       # each adds its option to the last


@pytest.fixture(scope="module")
def model():
    net, d = build_diffusion("C2", dim=DIM, device=DEV)
    assert [d._coef_table(S)[t].mode for t in TS] == [1, 1, 2]
    return net, d


class _Case:
    """The inputs and maps of one shape, centre size; `ext` wraps the last axis by `hx` as the library wants them."""

    def __init__(self, model, H, W):
        self.net, self.d = model
        rnd = lambda shape, key, a: (hash_randn(shape, key) * a).clamp(-1, 1).to(DEV)
        self.x0, self.xt = (hash_randn((B, 3, H, W), 1) * 0.8).to(DEV), rnd((B, 3, H, W), 2, 0.5)
        self.ew, self.ec = rnd((H, W), 3, 1.0).abs(), rnd((3, H, W), 4, 0.6)
        self.km, self.kx = (rnd((H, W), 5, 1.0) > 0).float(), rnd((3, H, W), 6, 0.6)
        self.lay = rnd((3, H, W), 7, 0.6)
        self.seeds = torch.tensor([11, 2 ** 40 + 5, 77], dtype=torch.int64, device=DEV)
        n = len(TS)
        tab, ab = self.d._coef_table(S), self.d._keep_ab_table()
        self.coefs, self.tl = (_lib.StepCoefs * n)(*[tab[t] for t in TS]), (C.c_int * n)(*TS)
        self.ab = (C.c_float * (2 * n))(*[float(v) for t in TS for v in ab[t]])
        self.jumps = (_lib.JumpCoefs * n)(_lib.JumpCoefs(1, *self.d._jump_table(S)(TS[0] - 1, TS[0] + 1)), _lib.JumpCoefs(), _lib.JumpCoefs())
        self.g = (C.c_float * n)(0.0, 0.5, 1.0)                  # (no pull on the step that jumps)

    def run(self, level, as_batch, *, seed=99, sid0=0, edit=False, hx=0, keep=False, seeds=False, jumps=False, lay=False):
        """ENTRIES[level] with the options given -- or, `as_batch`, sinddm_sample_chain_batch with the same options and NULL for
        the blocks that entry does not have.  Returns the centre of the result."""
        lib, d = _lib.load(), self.d
        ext = lambda t: d._wrap_pad(t, 0, hx) if hx else t.contiguous()
        xa, xt = ext(self.x0).clone(), ext(self.xt)
        xb, eps = torch.empty_like(xa), torch.empty_like(xa)
        H, W = self.x0.shape[2:]
        ws = _workspace(DEV, lib.sinddm_workspace_bytes(DIM, B, H, W + 2 * hx))
        flag = C.c_int(-1)
        held = [ext(t) for t in (self.ew, self.ec, self.km, self.kx, self.lay)]
        delta = torch.empty(B * 3 * (-(-H // 4)) * (-(-W // 4)), device=DEV)
        opts = _lib.ChainOpts(_lib.ptr(held[0]), _lib.ptr(held[1]), None) if edit else None
        kopts = _lib.KeepOpts(_lib.ptr(held[2]), _lib.ptr(held[3]), C.cast(self.ab, C.POINTER(C.c_float))) if keep else None
        ropts = _lib.ResampleOpts(self.jumps, None) if jumps else None
        lopts = _lib.LayoutOpts(_lib.ptr(held[4]), 4, C.cast(self.g, C.POINTER(C.c_float)), _lib.ptr(delta)) if lay else None
        ref = lambda o: C.byref(o) if o is not None else None
        args = [_lib.ptr(self.net.flat_params), _lib.ptr(self.net.packed_weights()), _lib.ptr(xa), _lib.ptr(xb), _lib.ptr(eps),
                _lib.ptr(xt), self.coefs, self.tl, len(TS), float(S), seed, sid0, DIM, B, H, W, ws.data_ptr(), ws.numel(),
                _lib.stream_ptr(DEV), None, C.byref(flag)]
        tail = [ref(opts), 0, hx, ref(kopts), _lib.ptr(self.seeds) if seeds else None, ref(ropts), ref(lopts), None]
        if as_batch:
            level = len(ENTRIES) - 1
        if level == 0:
            del args[-2]                                        # (sinddm_sample_chain has no aux_stream)
        rc = getattr(lib, "sinddm_sample_chain" + ENTRIES[level])(*args, *tail[:(0, 0, 1, 3, 4, 5, 6, 7, 8)[level]])
        torch.cuda.synchronize()
        assert rc == 0 and flag.value in (0, 1)
        y = xb if flag.value == 1 else xa
        assert bool(torch.isfinite(y).all())
        return y[..., hx:hx + W].contiguous()


# what each entry is called with: the richest set of options its signature has
OPTIONS = [dict(), dict(), dict(edit=True), dict(edit=True, hx=HALO), dict(edit=True, hx=HALO, keep=True),
           dict(edit=True, keep=True, seeds=True), dict(edit=True, hx=HALO, keep=True, seeds=True, jumps=True),
           dict(edit=True, keep=True, seeds=True, lay=True)]


@pytest.mark.parametrize("H,W", [(8, 12), (5, 7)], ids=["fused_8x12", "unfused_5x7"])
def test_narrow_entries_are_the_batch_entry(model, H, W):
    c = _Case(model, H, W)
    plain = c.run(0, False)
    seen = [plain]
    for level, kw in enumerate(OPTIONS):
        y = c.run(level, False, **kw)
        assert torch.equal(y, c.run(level, True, **kw)), ENTRIES[level]
        if level >= 2:
            assert not any(torch.equal(y, z) for z in seen), ENTRIES[level]      # (the option did something)
            seen.append(y)
    assert torch.equal(c.run(1, False), plain)


@pytest.mark.parametrize("H,W", [(8, 12), (5, 7)], ids=["fused_8x12", "unfused_5x7"])
def test_run_steps_is_the_narrow_entry_of_its_route(model, H, W):
    """`_run_steps` (sinddm_sample_chain_batch for every route) against the narrowest entry that can express the route: plain ->
    sinddm_sample_chain_ex, tiled -> _tile, keep maps -> _keep, per-sample seeds -> _seeds."""
    c = _Case(model, H, W)
    d = c.d
    d.img_prev_upsample, d.two_streams = c.xt, False
    routes = [("plain", 2, dict(), dict()), ("tiled", 3, dict(tile=(False, True)), dict(hx=HALO)),
              ("keep", 4, dict(keep_maps={S: (c.km, c.kx)}), dict(keep=True)),
              ("seeds", 5, dict(sample_seeds=c.seeds.tolist()), dict(seeds=True, sid0=noise_stream_id(S, "step", 0), seed=0))]
    try:
        for name, level, attrs, kw in routes:
            for k, v in attrs.items():
                setattr(d, k, v)
            torch.manual_seed(11)
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
            torch.manual_seed(11)
            got = d._run_steps(c.x0.clone(), S, TS)
            assert torch.equal(got, c.run(level, False, **{"seed": seed, **kw})), name
            d.tile, d.keep_maps, d.sample_seeds = (False, False), None, None
    finally:
        d.tile, d.keep_maps, d.sample_seeds, d.img_prev_upsample = (False, False), None, None, None
