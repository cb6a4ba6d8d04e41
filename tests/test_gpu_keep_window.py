"""Windowed known-region sampling on the GPU (MultiScaleGaussianDiffusion.keep_window, sinddm_normal_fill_window).

  4. the fill, bit for bit: every slot of sinddm_normal_fill_window is the slice of sinddm_normal_fill_samples / _mix at the
     window's absolute position, for unaligned sizes, per-sample origins, K = 1 and K = 3; nothing outside `out` is written;
  5. the windowed chain is the full chain (fused route): known pixels and everything outside the windows bit for bit -- which
     proves the draws --, free pixels within twice what the library's own two conv routes differ by; a window without its
     margin is not; one and two streams are bit-equal;
  6. routes and options: fused windowed = stepwise windowed, `resample` with a jump, `keep_gated`;
  7. `inpaint(..., window=16)` on the C1 pyramid against the same call without.
The yardstick of 5 / 6 (b): e = max|windowed - full| on the free pixels against r = max|full - full with fp32_convs|, the
parent's own two kernel routes on the same inputs; e <= 2 r + 4e-6 max(1, |full|max) (a window may change both the conv route
and the Winograd tile phase; the additive term is test_gpu_keep._bound) and, independently, rel-L2 <= 1e-4."""
import pytest
import torch

from conftest import max_abs, rel_l2
from sinddm_amd.synth import hash_randn
from test_gpu_chain_guided import _setup, _trainer
from test_gpu_keep import _bound, _known

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- 4: the fill -----------------------------------------------------------------------------------------------------------
FH, FW, FB = 13, 18, 3                                                     # 3 H W % 4 == 2, W % 4 == 2
SEEDS = [11, (1 << 62) + 5, 987654321]
MIX_KEYS = [[11, 12, 13], [21, 22, 23], [31, 32, 33]]
MIX_W = [[0.6, 0.0, 0.8], [0.36, 0.48, 0.8], [1.0, 0.0, 0.0]]             # (one zero weight in a row: that stream is skipped)


def _ids():
    from sinddm_amd import _lib
    return [(2 << 32) | 5, (2 << 32) | 6, (2 << 32) | (_lib.JUMP_STREAM + 2 + 3)]


def _full(sid, mix):
    """(B, 3, H, W): the draws of the whole samples at stream id `sid`."""
    from sinddm_amd import _lib
    lib = _lib.load()
    n = 3 * FH * FW
    out = torch.empty(FB * n, device=DEV)
    if mix:
        k, w = torch.tensor(MIX_KEYS, dtype=torch.int64, device=DEV), torch.tensor(MIX_W, dtype=torch.float32, device=DEV)
        _lib.check(lib.sinddm_normal_fill_mix(_lib.ptr(out), FB, n, _lib.ptr(k), _lib.ptr(w), 3, sid, _lib.stream_ptr(DEV)), "mix")
    else:
        k = torch.tensor(SEEDS, dtype=torch.int64, device=DEV)
        _lib.check(lib.sinddm_normal_fill_samples(_lib.ptr(out), FB, n, _lib.ptr(k), sid, _lib.stream_ptr(DEV)), "samples")
    torch.cuda.synchronize()
    return out.view(FB, 3, FH, FW)


def _window_fill(ids, origins, h, w, mix, unit_weights=False):
    """sinddm_normal_fill_window into the middle of a larger buffer: (the slots, whether the guard floats survived)."""
    from sinddm_amd import _lib
    lib = _lib.load()
    n, guard = len(ids) * FB * 3 * h * w, 64
    buf = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    out = buf[guard:guard + n]
    idt = torch.tensor(ids, dtype=torch.int64, device=DEV)
    org = torch.tensor(origins, dtype=torch.int32, device=DEV)
    if mix:
        k, wt = torch.tensor(MIX_KEYS, dtype=torch.int64, device=DEV), torch.tensor(MIX_W, dtype=torch.float32, device=DEV)
    else:
        k = torch.tensor(SEEDS, dtype=torch.int64, device=DEV)[:, None].contiguous()
        wt = torch.ones(FB, 1, device=DEV) if unit_weights else None
    rc = lib.sinddm_normal_fill_window(out.data_ptr(), len(ids), _lib.ptr(idt), FB, FH, FW, _lib.ptr(org), h, w, _lib.ptr(k),
                                       _lib.ptr(wt), int(k.shape[1]), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0
    intact = bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())
    return out.view(len(ids), FB, 3, h, w), intact


@pytest.mark.parametrize("mix", [False, True], ids=["K1", "K3"])
@pytest.mark.parametrize("h,w,origins", [(6, 7, [(3, 5), (0, 0), (7, 11)]), (FH, FW, [(0, 0)] * 3), (1, 1, [(12, 17), (0, 0), (5, 9)]),
                                         (FH, 3, [(0, 15), (0, 0), (0, 2)])],
                         ids=["6x7", "whole", "1x1", "column"])
def test_fill_window_is_the_slice_of_the_fill(h, w, origins, mix):
    ids = _ids()
    got, intact = _window_fill(ids, origins, h, w, mix)
    assert intact and torch.isfinite(got).all()
    for i, sid in enumerate(ids):
        full = _full(sid, mix)
        for b, (oy, ox) in enumerate(origins):
            assert torch.equal(got[i, b], full[b, :, oy:oy + h, ox:ox + w]), (i, b)
    if (h, w) == (FH, FW):                                                 # the window that spans the sample IS the plain fill
        assert torch.equal(got[0], _full(ids[0], mix))
    if not mix:                                                            # K = 1 with weight 1 is the seed itself, bit for bit
        assert torch.equal(_window_fill(ids, origins, h, w, False, unit_weights=True)[0], got)
    # the slots differ from each other and the samples from each other
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0], got[2]) and not torch.equal(got[0, 0], got[0, 1])


def test_fill_window_clamps_its_origins_and_refuses_bad_arguments():
    from sinddm_amd import _lib
    lib = _lib.load()
    ids = _ids()[:1]
    # origins outside the range the caller guarantees are clamped into it: nothing outside `out` is touched
    got, intact = _window_fill(ids, [(100, -5), (-3, 40), (7, 11)], 6, 7, False)
    ref, _ = _window_fill(ids, [(FH - 6, 0), (0, FW - 7), (7, 11)], 6, 7, False)
    assert intact and torch.equal(got, ref)
    # argument errors: their codes, and no launch (`out` keeps its NaNs)
    out = torch.full((FB * 3 * 6 * 7,), float("nan"), device=DEV)
    idt, org = torch.tensor(ids, dtype=torch.int64, device=DEV), torch.zeros(FB, 2, dtype=torch.int32, device=DEV)
    k, st = torch.tensor(SEEDS, dtype=torch.int64, device=DEV), _lib.stream_ptr(DEV)
    call = lambda **kw: lib.sinddm_normal_fill_window(*[{**dict(out=_lib.ptr(out), n=1, ids=_lib.ptr(idt), B=FB, H=FH, W=FW,
                                                                 org=_lib.ptr(org), h=6, w=7, keys=_lib.ptr(k), wts=None, K=1), **kw}[a]
                                                        for a in ("out", "n", "ids", "B", "H", "W", "org", "h", "w", "keys", "wts", "K")], st)
    assert call(out=None) == call(ids=None) == call(org=None) == call(keys=None) == -1
    assert call(K=2) == -1 and call(K=0) == -1 and call(K=5) == -1         # (K = 2 without weights)
    assert call(keys=_lib.ptr(k) + 4) == -1 and call(ids=_lib.ptr(idt) + 4) == -1 and call(out=_lib.ptr(out) + 2) == -1
    assert call(n=0) == call(B=0) == call(h=0) == call(w=-1) == -1
    assert call(h=FH + 1) == call(w=FW + 1) == call(B=65536) == call(H=32768, W=32768) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ---- 5, 6: the windowed chain ----------------------------------------------------------------------------------------------
class _Case:
    """One shape with keep maps; `run` is `_run_steps` under a setting of `keep_window` / streams / conv route."""

    def __init__(self, cfg, dim, s, B, mask, gated=False):
        self.net, self.d, self.H, self.W, self.x0, self.xt, _, _ = _setup(cfg, dim, s, B)
        self.s, self.B = s, B
        if s == 0:
            self.d.img_prev_upsample = None
        self.m = mask(self.H, self.W).to(DEV)
        self.k0 = _known(self.H, self.W)
        d = self.d
        d.keep_maps, d.keep_gated, d.sample_seeds = {s: (self.m, self.k0)}, gated, [101 + 7 * b for b in range(B)]
        mm = self.m if self.m.dim() == 3 else self.m[None].expand(B, -1, -1)
        self.known = (mm == 1)[:, None].expand(-1, 3, -1, -1)
        self.free = ~self.known

    def run(self, ts, window=None, two_streams=True, fp32=False, log=None):
        d = self.d
        d.keep_window, d.two_streams, d.draw_log, self.net.fp32_convs = window, two_streams, log, fp32
        try:
            y = d._run_steps(self.x0.clone(), self.s, ts)
            torch.cuda.synchronize()
        finally:
            d.keep_window, d.two_streams, d.draw_log, self.net.fp32_convs = None, True, None, False
        assert torch.isfinite(y).all()
        return y

    def compare(self, tag, win, full, full32):
        """(a) and (b) of the module docstring; returns e."""
        assert bool(self.known.any()) and bool(self.free.any())
        assert torch.equal(win[self.known], full[self.known])              # (a): the draws, and what `leave` puts outside
        e, r = max_abs(win[self.free].cpu(), full[self.free].cpu()), max_abs(full[self.free].cpu(), full32[self.free].cpu())
        bound = 2.0 * r + _bound(full)
        l2 = rel_l2(win[self.free].cpu(), full[self.free].cpu())
        print(f"{tag}: windowed vs full on the free pixels e = {e:.3e}, the two conv routes r = {r:.3e} (bound {bound:.3e}), "
              f"rel-L2 {l2:.3e}")
        assert e <= bound
        assert l2 <= 1e-4
        return e


def _hole_a(H, W):
    m = torch.ones(H, W)
    m[40:60, 60:84] = 0                                                    # a hard 20x24 hole ...
    m[44:50, 84:90] = 0.25                                                 # ... plus a soft patch
    return m


def _holes_a2(H, W):
    m = torch.stack([_hole_a(H, W), torch.ones(H, W)])
    m[1, 110:122, 150:165] = 0                                             # the second sample: another hole, its grown box
    m[1, 115, 165] = 0.5                                                   # clipped at the bottom and at the right border
    return m


def _hole_b(H, W):
    m = torch.ones(H, W)
    m[21:27, 30:38] = 0                                                    # 6x8
    return m


CHAIN = [("C2", 160, 3, 2, [311, 2, 0], _hole_a, (52, 64)), ("C2", 160, 3, 2, [311, 2, 0], _holes_a2, (52, 64)),
         ("C2", 160, 0, 4, [700, 2, 0], _hole_b, (38, 40))]
CHAIN_IDS = ["133x177_shared_hole", "133x177_two_holes", "48x64_mode0"]


@pytest.mark.parametrize("cfg,dim,s,B,ts,mask,hw", CHAIN, ids=CHAIN_IDS)
def test_windowed_chain_is_the_full_chain(cfg, dim, s, B, ts, mask, hw):
    c = _Case(cfg, dim, s, B, mask)
    full, full32 = c.run(ts), c.run(ts, fp32=True)
    log = []
    win = c.run(ts, window=16, log=log)
    assert len(log) == 1 and log[0][0] == "chain_window" and log[0][1:4] == (s, c.d.sample_seeds, ts) and log[0][4] is None
    assert log[0][5] == hw and tuple(log[0][6].shape) == (B, 2)
    e = c.compare(f"{cfg} dim {dim} s={s} {c.H}x{c.W} B={B} window {hw}", win, full, full32)
    # (c) the control: the window without its margin is another picture
    win0 = c.run(ts, window=0)
    e0 = max_abs(win0[c.free].cpu(), full[c.free].cpu())
    print(f"    margin 0: {e0:.3e}")
    assert e0 > 10.0 * e
    assert torch.equal(win0[c.known], full[c.known])                       # (its known pixels are still the full run's)
    # (d) one stream and two streams
    assert torch.equal(c.run(ts, window=16, two_streams=False), win)
    # the image of a seed does not depend on its batch: sample 1 alone, windowed
    c.d.sample_seeds = c.d.sample_seeds[1:2]
    x0, xt, m = c.x0, c.d.img_prev_upsample, c.m
    c.x0, c.d.img_prev_upsample = x0[1:2].contiguous(), xt[1:2].contiguous() if xt is not None else None
    if m.dim() == 3:
        c.d.keep_maps = {s: (m[1:2].contiguous(), c.k0)}
    one = c.run(ts, window=16)
    k1, f1 = c.known[1:2], c.free[1:2]
    assert torch.equal(one[k1], full[1:2][k1])
    assert max_abs(one[f1].cpu(), full[1:2][f1].cpu()) <= 2.0 * max_abs(full[c.free].cpu(), full32[c.free].cpu()) + _bound(full)


def test_windowed_fused_equals_windowed_stepwise():
    """ROI guidance on (its maps are gathered through the windows too): `chain_guided` picks the route."""
    def hole(H, W):
        m = torch.ones(H, W)
        m[10:30, 20:44] = 0                                                # (the window overlaps two of the ROI boxes)
        m[12, 44] = 0.5
        return m
    c, ts = _Case("C2", 160, 3, 2, hole), [311, 2, 0]
    d = c.d
    d.roi_guided_sampling = True
    try:
        log = []
        fused = c.run(ts, window=16, log=log)
        assert [e[0] for e in log] == ["chain_window"]
        d.chain_guided = False
        log = []
        step = c.run(ts, window=16, log=log)
        assert [e[0] for e in log] == ["step"] * len(ts) and tuple(log[0][3].shape) == (2, 3, 46, 60)
        err, bound = max_abs(fused.cpu(), step.cpu()), _bound(step)
        print(f"windowed fused vs windowed stepwise (ROI on) max-abs {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert torch.equal(fused[c.known], step[c.known])
        d.chain_guided = True
        c.compare("ROI on, 133x177 window (46, 60)", fused, c.run(ts), c.run(ts, fp32=True))
        d.roi_guided_sampling = False
        assert max_abs(c.run(ts, window=16)[c.free].cpu(), fused[c.free].cpu()) > 1e-3      # (the ROI maps acted in the window)
    finally:
        d.roi_guided_sampling, d.chain_guided = False, True


def test_windowed_resample_with_a_jump():
    c, ts = _Case("C2", 160, 3, 2, _holes_a2), [5, 4, 3, 2, 1, 0]
    c.d.omega = 0.3
    c.d.resample = (2, 2)
    try:
        log = []
        win = c.run(ts, window=16, log=log)
        assert log[0][0] == "chain_window" and any(j is not None for j in log[0][4]) and len(log[0][3]) > len(ts)
        c.compare("resample (2, 2), 133x177 two holes", win, c.run(ts), c.run(ts, fp32=True))
    finally:
        c.d.resample = None


def test_windowed_gated_run():
    def hold(H, W):
        h = torch.ones(H, W)
        h[40:60, 60:84] = 0.0                                              # redrawn from the top
        h[44:52, 84:92] = 0.4                                              # released on the way down
        h[60:64, 60:70] = 0.8
        return h
    c, ts = _Case("C2", 160, 3, 2, hold, gated=True), list(range(7, -1, -1))
    c.d.omega = 0.3
    win, full = c.run(ts, window=16), c.run(ts)
    c.compare("keep_gated, 133x177", win, full, c.run(ts, fp32=True))
    c.d.keep_gated = False
    assert max_abs(c.run(ts, window=16)[c.free].cpu(), win[c.free].cpu()) > 1e-3             # (the gate acted in the window)


@pytest.mark.parametrize("s,ts,mask", [(3, [311, 2], _holes_a2), (0, [700, 2], _hole_b)], ids=["mode1", "mode0"])
def test_windowed_run_that_does_not_land_clean(s, ts, mask):
    """The run ends on level 1: outside the windows the full run holds ka * target + kb * z of its last draw, not the known
    image -- `leave` computes that value at full size."""
    c = _Case("C2", 160, s, 2, mask)
    c.d.omega = 0.3
    full = c.run(ts)
    assert not torch.equal(full[c.known], c.k0[None].expand(2, -1, -1, -1)[c.known])
    c.compare(f"ends on level {ts[-1] - 1}, s={s}", c.run(ts, window=16), full, c.run(ts, fp32=True))


def test_unseeded_windowed_run_is_keyed_per_sample():
    c, ts = _Case("C2", 160, 0, 4, _hole_b), [700, 2, 0]
    c.d.sample_seeds = None
    torch.manual_seed(77)
    seeds = torch.randint(0, 2 ** 62, (4,), dtype=torch.int64).tolist()
    torch.manual_seed(77)
    log = []
    y = c.run(ts, window=16, log=log)
    assert log[0][0] == "chain_window" and log[0][2] == seeds
    c.d.sample_seeds = seeds
    assert torch.equal(c.run(ts, window=16), y)


# ---- 7: the public API -------------------------------------------------------------------------------------------------------
def test_inpaint_with_a_window_on_c1(golden, tmp_path):
    from sinddm_amd.functions import keep_mask_pyramid, keep_windows
    tr, meta = _trainer(golden, tmp_path)
    em = tr.ema_model
    sizes = [tuple(s) for s in meta["image_sizes_hw"]]
    H, W = sizes[-1]
    mask = torch.ones(H, W)
    mask[28:64, 24:104] = 0                                                # (scale 0's window spans the scale: it runs as ever)
    kw = dict(batch_size=2, seeds=[5, 6], custom_t_list=em.num_timesteps_ideal[1:], save_images=False)
    full = tr.inpaint(mask, **kw)
    em.draw_log = []
    win = tr.inpaint(mask, window=16, **kw)
    log, em.draw_log = em.draw_log, None
    assert em.keep_window is None and em.keep_maps is None
    masks = keep_mask_pyramid(mask, sizes, hard=True)
    small = [keep_windows(m < 1, 16) is not None for m in masks]
    assert small == [False, True, True]
    assert [e[0] for e in log if e[0].startswith("chain")] == ["chain_window" if w else "chain_seeds" for w in small]
    for s, (a, b) in enumerate(zip(win, full)):
        err = rel_l2(a.cpu(), b.cpu())
        print(f"inpaint C1 scale {s} {sizes[s]} window {small[s]}: windowed vs full rel-L2 {err:.3e}")
        assert err <= 1e-4
        kept = (masks[s] == 1).to(DEV)
        assert torch.equal(a[:, :, kept], b[:, :, kept])
    img = tr.data_list[-1][0][0]
    kept = mask.bool().to(DEV)
    assert torch.equal(win[-1][:, :, kept], img[None].expand(2, -1, -1, -1)[:, :, kept])
    assert max_abs(win[-1][0][:, ~kept].cpu(), win[-1][1][:, ~kept].cpu()) > 1e-2
