"""sampler.RunPlan on the CPU: the one host-side description of a run of reverse steps that both routes of `_run_steps` consume.
C2 at dim 20 on CPU tensors, B = 3 on 8x12, scales 0 and 1, the ten levels [9 .. 0].  For every sampler option alone and every
pair of them that is built:
  1. every step record equals, field for field, what the pinned helpers give when called here, independently of the plan
     (`_coef_table` / `step_coefs_to`, `_keep_ab_table`, `_jump_table`, functions.layout_strengths, `_solver_q`, and the
     schedules of functions.stride_schedule / resample_schedule);
  2. `pack_steps` of a piece [i0, i0 + k) is those records byte for byte, for three different cuts of the run;
  3. the one-step plan `_p_sample_host_t` builds for position i holds the same record as record i of the run's plan;
  4. each combination that is not built, each malformed option and each mismatching map raises from the constructor, with
     the exception type the option readers have always raised."""
import ctypes as C
import itertools
import struct

import pytest
import torch

from sinddm_amd import _lib, models
from sinddm_amd.configs import build_diffusion
from sinddm_amd.functions import layout_strengths, resample_schedule, stride_schedule
from sinddm_amd.sampler import NOT_BUILT, RunPlan, pack_steps

B, H, W, T_SEQ = 3, 8, 12, list(range(9, -1, -1))
OPTS = {
    "roi": lambda s: dict(roi_guided_sampling=True, roi_bbs=[[4, 8, 12, 16]],
                          roi_target_patch=[torch.full((1, 3, 4, 5), 0.1 * i) for i in range(5)]),
    "tile": lambda s: dict(tile=(False, True)),
    "keep": lambda s: dict(keep_maps={s: (torch.ones(H, W), torch.zeros(3, H, W))}),
    "keep_b": lambda s: dict(keep_maps={s: (torch.ones(B, H, W), torch.zeros(3, H, W))}),
    "resample": lambda s: dict(resample=(2, 2)),
    "layout": lambda s: dict(layout_maps={s: torch.zeros(3, H, W)}, layout_down={s: 3}, layout_strength=0.75, layout_t_min=4),
    "layout_gain": lambda s: dict(layout_maps={s: torch.zeros(B, 3, H, W)}, layout_down={s: 3}, layout_strength={s: 0.5},
                                  layout_t_min={s: 4}, layout_gain=[0.5, 1.0, 0.25]),
    "steps4_t": lambda s: dict(sample_steps=4, sample_spacing="t"),
    "steps4_logsnr": lambda s: dict(sample_steps=4, sample_spacing="logsnr"),
    "order2": lambda s: dict(solver_order=2),
    "eta0": lambda s: dict(eta=0.0),
}
FAMILY = {"keep_b": "keep", "layout_gain": "layout", "steps4_logsnr": "steps4_t"}
FEW = {"steps4_t", "steps4_logsnr", "order2", "eta0"}


def _built(a, b):
    """Whether the pair of options is one the sampler builds (the issue's list: layout with resample, order 2 with layout or
    resample, few-step with resample are not)."""
    fam = {FAMILY.get(a, a), FAMILY.get(b, b)}
    if len(fam) == 1:
        return False
    return not (fam == {"layout", "resample"} or fam == {"layout", "order2"} or ("resample" in fam and fam & FEW))


SETTINGS = [()] + [(o,) for o in OPTS] + [p for p in itertools.combinations(OPTS, 2) if _built(*p)]


@pytest.fixture(scope="module")
def model():
    net, d = build_diffusion("C2", dim=20, device="cpu")
    d.omega = 0.3
    d.img_prev_upsample = torch.zeros(B, 3, H, W)
    return d


@pytest.fixture
def configured(model):
    """set(names, s) puts the options on the model; everything is put back afterwards."""
    saved = {}

    def put(names, s, **extra):
        for kw in [OPTS[o](s) for o in names] + [extra]:
            for k, v in kw.items():
                saved.setdefault(k, getattr(model, k))
                setattr(model, k, v)
        return model
    yield put
    for k, v in saved.items():
        setattr(model, k, v)


def _fields(st):
    return (st.pos, st.t, st.land, bytes(st.k), st.ab, st.jump_to, None if st.jump is None else bytes(st.jump), st.g, st.q)


def _expected(d, s, img):
    """The records of the run from the pinned helpers alone, as `_fields` tuples."""
    t_seq, lands, q = list(T_SEQ), None, None
    few = d._few_step_cfg(s)
    if few is not None:
        t_seq, lands = stride_schedule(t_seq, few[0] if few[0] is not None else len(t_seq), few[1], d._kappa(s))
        q = d._solver_q(s, t_seq, lands) if few[2] == 2 else None
    jump_to = [None] * len(t_seq)
    if d._resample_cfg() is not None:
        t_seq, jump_to = resample_schedule(t_seq, *d._resample_cfg())
    lay = d._layout_entry(s, img)
    g = layout_strengths(t_seq, lay[2], lay[3]) if lay is not None else [0.0] * len(t_seq)
    keep = d._keep_entry(s, img) is not None
    out = []
    for i, t in enumerate(t_seq):
        land = t - 1 if lands is None else lands[i]
        k = d._coef_table(s)[t] if lands is None else d.step_coefs_to(t, land, s, eta=d.eta)
        ab = tuple(float(v) for v in d._keep_ab_table()[land + 1]) if keep else (1.0, 0.0)
        jump = None if jump_to[i] is None else bytes(_lib.JumpCoefs(1, *d._jump_table(s)(t - 1, jump_to[i])))
        out.append((i, t, land, bytes(k), ab, jump_to[i], jump, g[i], None if q is None else q[i]))
    return out


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("names", SETTINGS, ids=lambda n: "+".join(n) or "plain")
def test_records_packing_and_one_step_plans(configured, monkeypatch, names, s):
    d = configured(names, s)
    img = torch.zeros(B, 3, H, W)
    plan = RunPlan(d, img, s, T_SEQ)
    want = _expected(d, s, img)
    n = len(want)
    # 1: the records
    assert [_fields(st) for st in plan.steps] == want
    assert plan.t_seq == [w[1] for w in want] and [st.k.mode for st in plan.steps] == ([0] * n if s == 0 else [1] * (n - 1) + [2])
    assert (plan.jump_to is not None) == ("resample" in names) and plan.order2 == ("order2" in names)
    assert plan.halo == ((0, _lib.TILE_HALO) if "tile" in names else (0, 0))
    assert (plan.roi is not None) == ("roi" in names) and (plan.keep is not None) == bool({"keep", "keep_b"} & set(names))
    assert (plan.lay is not None) == bool({"layout", "layout_gain"} & set(names))
    assert plan.per == (0, int("keep_b" in names), 0, int("layout_gain" in names))
    assert (plan.gain.tolist() if plan.gain is not None else None) == ([0.5, 1.0, 0.25] if "layout_gain" in names else None)
    assert plan.noise == ("torch", None) and (plan.xt is not None) == (s > 0)
    if plan.lay is not None:                                                # (layout_t_min = 4 lies inside the run)
        assert [st.g > 0.0 for st in plan.steps] == [st.t >= 4 for st in plan.steps] and 0 < sum(st.g > 0 for st in plan.steps) < n
    # 2: packing, three cuts
    floats = lambda vals: struct.pack(f"{len(vals)}f", *vals)
    for i0, k in ((0, n), (0, 2), (2, n - 2), (1, 2)):                      # (the shortest run has 4 steps)
        p, recs = pack_steps(plan, i0, k), plan.steps[i0:i0 + k]
        assert bytes(p.coefs) == b"".join(bytes(r.k) for r in recs) and list(p.tl) == [r.t for r in recs]
        assert (None if p.ab is None else bytes(p.ab)) == (floats([v for r in recs for v in r.ab]) if plan.keep is not None else None)
        assert (None if p.jumps is None else bytes(p.jumps)) == (
            b"".join(bytes(r.jump if r.jump is not None else _lib.JumpCoefs(0, 0.0, 0.0, 0.0)) for r in recs)
            if "resample" in names else None)
        assert (None if p.g is None else bytes(p.g)) == (floats([r.g for r in recs]) if plan.lay is not None else None)
        assert (None if p.q is None else bytes(p.q)) == (floats([r.q for r in recs]) if plan.order2 else None)
        assert len(p.coefs) == len(p.tl) == k and C.sizeof(p.coefs) == k * C.sizeof(_lib.StepCoefs)
    # 3: the plan `_p_sample_host_t` builds for each position (it then stops at the network: there is no CPU fallback)
    built = []

    class Spy(RunPlan):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self)

    monkeypatch.setattr(models, "RunPlan", Spy)
    strided = d._few_step_cfg(s) is not None
    for st in plan.steps:
        with pytest.raises(_lib.SinddmError, match="no CPU fallback"):
            d._p_sample_host_t(img, st.t, s, step_pos=st.pos, jump_to=st.jump_to, land=st.land if strided else None, q=st.q,
                               hist=img if st.q is not None else None)
    assert [len(b.steps) for b in built] == [1] * n
    assert [_fields(b.steps[0]) for b in built] == want


def test_noise_source_and_log_entries(configured):
    d = configured((), 1)
    img = torch.zeros(B, 3, H, W)
    assert RunPlan(d, img, 1, [2, 1, 0]).log_entry(5) == ("chain", 1, 5, [2, 1, 0])
    d = configured(("tile",), 1)
    assert RunPlan(d, img, 1, [2, 1, 0]).log_entry(5) == ("chain_tile", 1, 5, [2, 1, 0], (0, _lib.TILE_HALO))
    d = configured(("resample",), 1, sample_seeds=[7, 8, 9])
    plan = RunPlan(d, img, 1, [2, 1, 0])
    assert plan.noise == ("seeds", [7, 8, 9])
    assert plan.log_entry(0) == ("chain_resample", 1, [7, 8, 9], plan.t_seq, plan.jump_to) and len(plan.t_seq) > 3
    d = configured((), 1, sample_seeds=None, resample=None, seed_mix=([[1, 2]] * B, [[0.6, 0.8]] * B))
    plan = RunPlan(d, img, 1, [2, 1, 0])
    assert plan.noise[0] == "mix" and plan.log_entry(0) == ("chain_mix", 1, plan.noise[1], [2, 1, 0], None)
    d = configured((), 1, seed_mix=None, sample_seeds=[7, 8, 9])
    assert RunPlan(d, img, 1, [2, 1, 0]).log_entry(0) == ("chain_seeds", 1, [7, 8, 9], [2, 1, 0])
    d = configured((), 1, sample_seeds=None, noise_fn=lambda *a: None)
    assert RunPlan(d, img, 1, [2, 1, 0]).noise == ("recorded", None)
    assert RunPlan(d, img, 1, []).steps == []                               # (an empty run is a plan without steps)


REFUSED = [(("keep",), dict(clip_guided_sampling=True)), (("layout",), dict(clip_guided_sampling=True)),
           (("resample",), dict(clip_guided_sampling=True)), (("steps4_t",), dict(clip_guided_sampling=True)),
           (("order2",), dict(clip_guided_sampling=True)), (("eta0",), dict(clip_guided_sampling=True)),
           ((), dict(clip_guided_sampling=True, seed_mix=([[1, 2]] * B, [[0.6, 0.8]] * B))),
           (("layout", "resample"), {}), (("order2", "layout"), {}), (("order2", "resample"), {}), (("steps4_t", "resample"), {})]
MALFORMED = [dict(solver_order=3), dict(sample_spacing="snr"), dict(eta=-0.5), dict(sample_steps=0), dict(resample=(0, 1)),
             dict(layout_maps={1: torch.zeros(3, H, W)}), dict(layout_maps={1: torch.zeros(3, H, W)}, layout_down={1: 65}),
             dict(layout_maps={1: torch.zeros(3, H, W)}, layout_down={1: 3}, layout_strength=1.5),
             dict(layout_maps={1: torch.zeros(3, H, W)}, layout_down={1: 3}, layout_gain=[0.5, 0.5]),
             dict(sample_seeds=[1, 2]), dict(sample_seeds=[1, 2, 3], seed_mix=([[1, 2]] * B, [[0.6, 0.8]] * B)),
             dict(seed_mix=([[1, 2]] * B, [[0.6, 0.6]] * B)), dict(roi_guided_sampling=True, roi_bbs_batch=[[[4, 8, 12, 16]]] * 2,
                                                                   roi_target_patch=[torch.zeros(1, 3, 4, 5)] * 5)]
MISMATCH = [dict(keep_maps={1: (torch.ones(H, W + 1), torch.zeros(3, H, W))}),
            dict(keep_maps={1: (torch.ones(H, W), torch.zeros(3, H, W, dtype=torch.float64))}),
            dict(layout_maps={1: torch.zeros(3, H + 1, W)}, layout_down={1: 3}), dict(img_prev_upsample=None)]


@pytest.mark.parametrize("names,extra,exc", [(n, e, NotImplementedError) for n, e in REFUSED]
                         + [((), e, ValueError) for e in MALFORMED] + [((), e, _lib.SinddmError) for e in MISMATCH])
def test_refusals_and_validation_raise_from_the_constructor(configured, names, extra, exc):
    d = configured(names, 1, **extra)
    with pytest.raises(exc) as err:
        RunPlan(d, torch.zeros(B, 3, H, W), 1, T_SEQ)
    assert type(err.value) is exc
    if exc is NotImplementedError:
        assert str(err.value) in NOT_BUILT.values()


def test_single_step_refusals(configured):
    d = configured((), 1)
    img = torch.zeros(B, 3, H, W)
    for at in ((0, 7, 4, None), (0, 7, None, 0.25)):                        # a strided / multistep step before a jump
        with pytest.raises(NotImplementedError):
            RunPlan(d, img, 1, [5], at=at)
    d = configured(("layout",), 1)
    for at in ((0, 7, None, None), (0, None, None, 0.25)):                  # a layout pull before a jump / on a multistep step
        with pytest.raises(NotImplementedError):
            RunPlan(d, img, 1, [5], at=at)
    assert RunPlan(d, img, 1, [3], at=(0, 7, None, None)).steps[0].g == 0.0   # (below layout_t_min the step does not pull)
    with pytest.raises(ValueError):
        d._p_sample_host_t(img, 5, 1, q=0.25)                               # q without hist
    d = configured((), 1, clip_guided_sampling=True)
    for at in ((0, 7, None, None), (0, None, 4, None)):
        with pytest.raises(NotImplementedError):
            RunPlan(d, img, 1, [5], at=at)
