"""Numpy reference of the windowed patch search (sinddm_patch_nnf_local): the yardstick of test_patch_local_host.py and
test_gpu_patch_local.py (test code, not product code).  Builds on nnf_util and refine_util."""
import numpy as np

import nnf_util as U
import refine_util as R

U24 = R.U24


def window_mask(prior, radius, ref_grid, wrap_r=(False, False)):
    """prior (M,) linear positions -> (M, N) bool: position j lies in the (2 radius + 1)^2 window of query i.  A prior < 0 or
    >= N has an empty window; a wrapped axis takes the window modulo the grid, an unwrapped one clips it."""
    hr, wr = ref_grid
    N = hr * wr
    prior = np.asarray(prior).reshape(-1).astype(np.int64)
    live = (prior >= 0) & (prior < N)
    py, px = np.where(live, prior, 0) // wr, np.where(live, prior, 0) % wr
    d = np.arange(-radius, radius + 1)
    ys, xs = py[:, None] + d[None], px[:, None] + d[None]                  # (M, 2R + 1) each
    yin, xin = np.zeros((len(prior), hr), bool), np.zeros((len(prior), wr), bool)
    rows = np.arange(len(prior))[:, None]
    for arr, inside, n, wrap in ((ys, yin, hr, wrap_r[0]), (xs, xin, wr, wrap_r[1])):
        if wrap:
            inside[rows, arr % n] = True
        else:
            on = (arr >= 0) & (arr < n)
            inside[np.broadcast_to(rows, arr.shape)[on], arr[on]] = True
    mask = yin[:, :, None] & xin[:, None, :]
    return (mask & live[:, None, None]).reshape(len(prior), N)


def local_field64(x, ref, P, prior, radius, wrap_q=(False, False), wrap_r=(False, False), ok=None, scale=None):
    """refine_util.field64 restricted per query to its window: (idx (M,), -1 where no candidate is left; D (M, N) float64 with
    +inf outside the window and where not admissible).  `scale` (N,): the winner minimises D * scale.  np.argmin takes the
    first of equal values: the smallest linear index."""
    _, D = R.field64(x, ref, P, wrap_q, wrap_r, ok=ok)
    hr, wr = U.grid(np.asarray(ref).shape[1:], P, wrap_r)
    D[~window_mask(prior, radius, (hr, wr), wrap_r)] = np.inf
    V = D if scale is None else D * np.asarray(scale, np.float64).reshape(1, -1)
    idx = V.argmin(axis=1)
    idx[~np.isfinite(V.min(axis=1))] = -1
    return idx, D


def check_local_field(query, ref, P, prior, radius, idx, dist, wrap_q=(False, False), wrap_r=(False, False), ok=None,
                      scale=None, what=""):
    """The criteria of the windowed field of ONE sample, for every query i with window W_i (admissible positions only):
      W_i empty: idx = -1 and dist = +inf; else the winner sel lies in W_i, and with K = 3 P^2, V = D64 (or D64 s_j):
      V(i, sel) - min_{j in W} V(i, j) <= e(sel) + e(jmin),   e(j) = (K + 4) 2^-24 D64(i, j)  [scaled: s_j (K + 5) 2^-24 D64]
      |dist - D64(i, sel)| <= (K + 4) 2^-24 D64(i, sel).
    These are the forward-error bounds of one K-step fmaf chain of non-negative terms (one more rounding for the scale's
    multiply).  Returns the worst ratio gap / bound."""
    idx = np.asarray(idx).reshape(-1).astype(np.int64)
    dist = np.asarray(dist, np.float64).reshape(-1)
    jmin, D = local_field64(query, ref, P, prior, radius, wrap_q, wrap_r, ok, scale)
    M, N = D.shape
    K = 3 * P * P
    assert idx.shape == (M,) and dist.shape == (M,), (what, idx.shape, dist.shape, M)
    none = jmin < 0
    assert np.array_equal(idx < 0, none), f"{what}: {int(((idx < 0) != none).sum())} queries differ in having a winner at all"
    assert (idx[none] == -1).all() and np.isposinf(dist[none]).all(), what
    rows = np.arange(M)[~none]
    sel, jm = idx[~none], jmin[~none]
    assert sel.max(initial=0) < N, (what, sel.max())
    dsel, dmin = D[rows, sel], D[rows, jm]
    assert np.isfinite(dsel).all(), f"{what}: {int((~np.isfinite(dsel)).sum())} winners outside the window or not admissible"
    if scale is None:
        gap, bound = dsel - dmin, (K + 4) * U24 * (dsel + dmin)
    else:
        s = np.asarray(scale, np.float64).reshape(-1)
        gap, bound = dsel * s[sel] - dmin * s[jm], (K + 5) * U24 * (s[sel] * dsel + s[jm] * dmin)
    derr, dbound = np.abs(dist[~none] - dsel), (K + 4) * U24 * dsel
    ratio = float((gap / np.maximum(bound, 1e-300)).max(initial=0.0))
    print(f"{what}: M {M} without a winner {int(none.sum())} worst gap / bound {ratio:.3f} worst dist ratio "
          f"{(derr / np.maximum(dbound, 1e-300)).max(initial=0.0):.3f} index mismatches {int((sel != jm).sum())}")
    assert (gap <= bound).all(), f"{what}: {int((gap > bound).sum())} queries beyond the bound, worst ratio {ratio:.3f}"
    assert (derr <= dbound).all(), f"{what}: {int((derr > dbound).sum())} distances beyond the bound"
    return ratio
