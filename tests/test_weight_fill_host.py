"""What a parity test can see depends on the weights it loads.  CPU only: everything here runs on the oracle.

`closed_form_state_dict` fills tensor k with a sin(0.37 i + k): since sin(A_co + B_j) = sin A_co cos B_j + cos A_co sin B_j,
every conv weight reshaped to (C_out, C_in k k) has rank 2, and at dim 160 the network's output is almost constant over the
image.  A kernel that reads its taps transposed, swaps two channels or pads one border wrongly then moves the output by
2e-5 .. 8e-5 of its norm -- next to a tolerance of 1e-5 on the whole tensor, of which one tile column or one channel chunk
is a small fraction.  With `he_state_dict` the same mutations move the output by 1e-2 .. 0.5.

  1. rank of both fills;
  2. the mutation table: on He weights every structural mutation moves the oracle's output by >= 100 x the tolerance the GPU
     forward tests of tests/test_gpu_fullrank.py apply, 3 x rel_l2(fp32 oracle, float64 oracle); on closed-form weights the
     same mutations stay under the upper bounds recorded here (so nobody "simplifies" the He tests back to closed-form);
  3. the same for the backward pass (tap transposition);
  4. the clip condition of the chain tests: with HE_EPS_GAIN fewer than 20 % of x_recon is clipped at their steps.
dim 160, input 2x3x37x41 (hash noise), t = [17, 503], scale 2.                     reference SinDDM/models.py:51-80,134-151
"""
import pytest
import torch

from conftest import rel_l2
from fullrank_util import (CHAIN_CFG, CHAIN_SCALE, CHAIN_TS, SPATIAL_MUTATIONS, WEIGHT_MUTATIONS, chain_inputs,
                           clipped_fraction, mutated_forward, net_forward_f64, oracle_autograd)
from oracle import sinddm_oracle as O
from sinddm_amd.configs import CONFIGS
from sinddm_amd.synth import HE_EPS_GAIN, closed_form_state_dict, hash_randn, he_state_dict, net_param_shapes

DIM, SCALE = 160, 2
_CACHE = {}


def _setup():
    """Both fills, the input, and the unmutated fp32 / float64 outputs -- computed once and left unchanged."""
    if not _CACHE:
        x, t = hash_randn((2, 3, 37, 41), 11), torch.tensor([17, 503])
        for fill, sd in (("closed_form", closed_form_state_dict(DIM)), ("he", he_state_dict(DIM))):
            with torch.no_grad():
                _CACHE[fill] = (sd, O.net_forward(sd, x, t, SCALE), net_forward_f64(sd, x, t, SCALE))
        _CACHE["x"], _CACHE["t"] = x, t
    return _CACHE


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_he_fill_is_what_the_tile_tests_loaded_and_eps_gain_touches_the_head_only():
    import numpy as np
    sd = he_state_dict(32)
    for k, (name, shape) in enumerate(net_param_shapes(32).items()):
        amp = 0.05 if name.endswith("bias") else float(np.sqrt(2.0 / int(np.prod(shape[1:]))))
        assert torch.equal(sd[name], hash_randn(shape, 1000 + k) * amp), name
    g = he_state_dict(32, eps_gain=0.25)
    for name in sd:
        assert torch.equal(g[name], sd[name] * 0.25 if name.startswith("final_conv.0.") else sd[name]), name
    assert not torch.equal(he_state_dict(32, key=7)["l1.net.0.weight"], sd["l1.net.0.weight"])


@pytest.mark.parametrize("name", ["l3.net.0.weight", "l3.net.2.weight", "l2.net.0.weight", "l2.net.2.weight", "l1.net.0.weight",
                                  "l2.res_conv.weight", "l4.res_conv.weight", "final_conv.0.weight"])
def test_rank_of_the_two_fills(name):
    """Closed-form 3x3 and 1x1 conv weights: numerical rank 2 (third singular value < 1e-6 of the first).  He: full rank --
    smallest / largest singular value > 0.3 for the 3x3 convs of the 160-channel blocks (0.36 .. 0.52), and for every tensor
    more than half of what a Gaussian m x n matrix has in the limit, (1 - sqrt(q)) / (1 + sqrt(q)) with q = min / max of
    (m, n) (Marchenko-Pastur: the ratio is set by the aspect ratio -- 0.17 for the 160 x 80 projection --, not by the fill)."""
    sv = {}
    for fill, f in (("closed_form", closed_form_state_dict), ("he", he_state_dict)):
        w = f(DIM)[name].double()
        sv[fill] = torch.linalg.svdvals(w.reshape(w.shape[0], -1))
    cf, he = sv["closed_form"], sv["he"]
    shape = net_param_shapes(DIM)[name]
    m, n = shape[0], shape[1] * shape[2] * shape[3]
    q = min(m, n) / max(m, n)
    mp = (1 - q ** 0.5) / (1 + q ** 0.5)
    print(f"{name} ({m} x {n}): closed-form s1/s0 {float(cf[1] / cf[0]):.3f} s2/s0 {float(cf[2] / cf[0]):.1e}; "
          f"He s2/s0 {float(he[2] / he[0]):.2f} smallest/largest {float(he[-1] / he[0]):.2f} (Gaussian limit {mp:.2f})")
    assert float(cf[1] / cf[0]) > 0.5 and float(cf[2] / cf[0]) < 1e-6
    assert float(he[-1] / he[0]) > 0.5 * mp
    if name in ("l3.net.0.weight", "l3.net.2.weight", "l2.net.0.weight", "l2.net.2.weight"):
        assert float(he[-1] / he[0]) > 0.3


def test_closed_form_output_forgets_its_input_he_output_does_not():
    c = _setup()
    x2 = hash_randn((2, 3, 37, 41), 12)
    with torch.no_grad():
        for fill, lo, hi in (("closed_form", 0.0, 1e-2), ("he", 0.3, 2.0)):
            sd, y, _ = c[fill]
            moved = rel_l2(O.net_forward(sd, x2, c["t"], SCALE), y)
            rms, sstd = float(y.pow(2).mean().sqrt()), float(y.std(dim=(2, 3)).mean())
            print(f"{fill}: output rms {rms:.3g}, mean spatial std {sstd:.3g}; another noise image moves it by {moved:.2e}")
            assert lo <= moved < hi, (fill, moved)
    assert float(c["closed_form"][1].std(dim=(2, 3)).mean()) < 0.01 * float(c["closed_form"][1].pow(2).mean().sqrt())
    assert float(c["he"][1].std(dim=(2, 3)).mean()) > 0.3 * float(c["he"][1].pow(2).mean().sqrt())


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
# mutation -> upper bound of what it moves the CLOSED-FORM output by (measured value in the comment).  1e-4 for the five of
# the table; the two spatial ones by their own measurements.
STRUCTURAL = {
    "transpose_taps_l3_net0": 1e-4,                 # 7.8e-5      (He: 0.48)
    "swap_in_channels_7_24_l3_net2": 1e-4,          # 6.9e-5      (He: 4.1e-2)
    "swap_out_channels_7_24_l2_net0": 1e-4,         # 3.5e-5      (He: 7.4e-2)
    "zero_one_tap_one_channel_l3_net0": 1e-4,       # 2.0e-5      (He: 1.2e-2)
    "replicate_right_l3_net0": 1e-5,                # 3.5e-6      (He: 2.8e-2)
    "shift_dw_l2": 1e-3,                            # 4.0e-4      (He: 0.52)
}


def _tolerance():
    """What tests/test_gpu_fullrank.py allows a forward: 3 x rel_l2(fp32 oracle, float64 oracle) on He weights."""
    _, y32, y64 = _setup()["he"]
    return 3 * rel_l2(y32, y64)


def test_mutations_are_the_ones_meant():
    assert set(STRUCTURAL) | {"truncate_l3_net2_to_16_mantissa_bits"} == set(WEIGHT_MUTATIONS) | set(SPATIAL_MUTATIONS)
    assert 1e-7 < _tolerance() < 1e-5, _tolerance()


@pytest.mark.parametrize("mutation", list(STRUCTURAL))
def test_structural_mutation_he_sees_it_closed_form_does_not(mutation):
    c = _setup()
    tol = _tolerance()
    with torch.no_grad():
        moved = {fill: rel_l2(mutated_forward(c[fill][0], c["x"], c["t"], SCALE, mutation), c[fill][1])
                 for fill in ("closed_form", "he")}
    print(f"{mutation}: closed-form output moves by {moved['closed_form']:.2e}, He by {moved['he']:.2e} "
          f"= {moved['he'] / tol:.0f} x the tolerance {tol:.2e}")
    assert moved["he"] >= 100 * tol, (mutation, moved, tol)
    assert 0 < moved["closed_form"] < STRUCTURAL[mutation], (mutation, moved)


def test_precision_mutation_16_mantissa_bits():
    """l3.net.2.weight truncated to 16 mantissa bits is not a structural error but a loss of width: it moves the He output by
    5.8e-6 -- 4.5 x the forward tolerance, so the He gate rejects it, but far from the 100 x margin of the structural
    mutations (the table this row comes from already says 5.8e-6; nothing of that size can be 100 x a tolerance of
    1.3e-6).  What holds and is asserted: above the tolerance, and an order of magnitude above what the closed-form network
    shows of it (5.2e-7: under ITS fp32-vs-float64 distance times 3, i.e. invisible there at any tolerance fp32 can meet)."""
    c = _setup()
    m = "truncate_l3_net2_to_16_mantissa_bits"
    with torch.no_grad():
        moved = {fill: rel_l2(mutated_forward(c[fill][0], c["x"], c["t"], SCALE, m), c[fill][1]) for fill in ("closed_form", "he")}
    tol = _tolerance()
    tol_cf = 3 * rel_l2(c["closed_form"][1], c["closed_form"][2])
    print(f"{m}: closed-form {moved['closed_form']:.2e} (3 x its fp32 error: {tol_cf:.2e}), He {moved['he']:.2e} "
          f"= {moved['he'] / tol:.1f} x the tolerance {tol:.2e}")
    assert moved["he"] > 3 * tol
    assert moved["he"] > 10 * moved["closed_form"]
    assert moved["closed_form"] < 1e-4 and moved["closed_form"] < tol_cf


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_backward_sees_the_tap_transposition_on_he_weights():
    """dim 160, 2x3x21x37: transposing l3.net.0's taps moves the He gradients of l2.net.0.weight, l1.ds_conv.weight and the
    input by > 0.1 each (closed-form: l2.net.0.weight 3.2e-2, final_conv.0.weight 6.6e-4); and the fp32 oracle's own worst
    gradient tensor sits 6e-5 from float64 on closed-form weights (cancellation: why those tests need 2e-4), under 1e-5 on He."""
    x, gy, t = hash_randn((2, 3, 21, 37), 5), hash_randn((2, 3, 21, 37), 6), torch.tensor([3, 14])
    for fill, sd in (("closed_form", closed_form_state_dict(DIM)), ("he", he_state_dict(DIM))):
        _, gx, g = oracle_autograd(sd, x, t, SCALE, gy, torch.float32)
        _, gx64, g64 = oracle_autograd(sd, x, t, SCALE, gy, torch.float64)
        worst32 = max(rel_l2(g[k], g64[k]) for k in g)
        s2 = dict(sd)
        WEIGHT_MUTATIONS["transpose_taps_l3_net0"](s2)
        _, gx2, g2 = oracle_autograd(s2, x, t, SCALE, gy, torch.float32)
        moved = {k: rel_l2(g2[k], g[k]) for k in ("l2.net.0.weight", "l1.ds_conv.weight", "final_conv.0.weight")}
        moved["input"] = rel_l2(gx2, gx)
        print(f"{fill}: fp32 oracle's worst gradient tensor vs float64 {worst32:.2e}; taps of l3.net.0 transposed: "
              + ", ".join(f"{k} {v:.2e}" for k, v in moved.items()))
        if fill == "he":
            assert moved["l2.net.0.weight"] > 0.1 and moved["l1.ds_conv.weight"] > 0.1 and moved["input"] > 0.1, moved
            assert worst32 < 1e-5
        else:
            assert moved["l2.net.0.weight"] < 0.05 and moved["final_conv.0.weight"] < 1e-3, moved
            assert worst32 > 2e-5


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (2, 13, 17)], ids=["2x24x40", "2x13x17"])
def test_clip_condition_of_the_chain_tests(B, H, W):
    """A condition on the INPUTS of the chain tests of tests/test_gpu_fullrank.py, checked on the oracle: with
    eps_gain = HE_EPS_GAIN[160] eps has an rms of about 1 and fewer than 20 % of x_recon are clipped at each step of
    CHAIN_TS; with eps_gain = 1 (rms ~40) more than 70 % are at the steps with t > 0 (measured 86 .. 98 %), which then hardly depend
    on eps.  The draws are hash
    noise here (the GPU test regenerates the library's own): the fraction is a property of their distribution."""
    cfg = CONFIGS[CHAIN_CFG]
    sched = O.make_schedule(cfg["T"], len(cfg["sizes"]), cfg["rescale_losses"], 1, train_full_t=True)
    s = CHAIN_SCALE
    x0, xt = chain_inputs(B, H, W)
    with torch.no_grad():
        for gain, ok in ((HE_EPS_GAIN[DIM], True), (1.0, False)):
            sd = he_state_dict(DIM, eps_gain=gain)
            x = x0
            for i, t in enumerate(CHAIN_TS):
                eps = O.net_forward(sd, x, torch.full((B,), t, dtype=torch.long), s)
                frac, rms = clipped_fraction(sched, x, eps, t, s, xt), float(eps.pow(2).mean().sqrt())
                print(f"{B}x{H}x{W} eps_gain {gain:g} t={t}: eps rms {rms:.3g}, clipped {100 * frac:.1f} %")
                if ok:
                    assert frac < 0.20, (t, frac)
                    assert 0.5 < rms < 2.0, (t, rms)
                elif t > 0:                                     # (at t = 0 eps enters x_recon with a factor of ~0.01)
                    assert frac > 0.7, (t, frac)
                x = O.reverse_step(sched, x, eps, t, s, hash_randn((B, 3, H, W), 63 + i), xt)
