"""Numpy references of the patch vote, the scaled patch field and the refinement loop: the yardsticks of
test_patch_refine_host.py and test_gpu_patch_refine.py (test code, not product code).  Builds on nnf_util (patch element
order (c, dy, dx), positions row-major)."""
import os

import numpy as np

import nnf_util as U

U24 = 2.0 ** -24
ALPHA = 0.005


def inputs(golden_dir):
    """The crops of balloons.png the tests run on, float32 in [-1, 1] (the query is left unclipped):
    query 3 x 22 x 26 = a crop + 0.3 N(0, 1), seed 3; ref 3 x 24 x 30; wide 3 x 30 x 80 (a reference row of two 64-position
    chunks, the second one partial, at every P)."""
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(golden_dir, "balloons.png")).convert("RGB"), dtype=np.float32)
    img = img.transpose(2, 0, 1) / 255.0 * 2.0 - 1.0
    noise = np.random.default_rng(3).normal(0.0, 1.0, (3, 22, 26))
    q = (img[:, 10:32, 20:46] + 0.3 * noise).astype(np.float32)
    r = img[:, 60:84, 100:130].copy()
    wide = img[:, 60:90, 40:120].copy()
    for a in (q, r, wide):
        a.setflags(write=False)
    return q, r, wide


# ---- the vote, float32, the kernel's add order and select rule ----

def vote_f32(idx, ref, base, P, wrap_q=(False, False), wrap_r=(False, False), weight=None, blend=1.0):
    """idx (h, w) int, ref (3, Hr, Wr), base (3, H, W), weight (H, W) or None -> (3, H, W) float32: sinddm_patch_vote of ONE
    sample.  Exact for g = blend * weight in {0, 1} or a power of two (g (mean - base) is then exact, so the fmaf is one
    rounding as the float32 add here is)."""
    ref, base = np.asarray(ref, np.float32), np.asarray(base, np.float32)
    _, H, W = base.shape
    _, Hr, Wr = ref.shape
    h, w = U.grid((H, W), P, wrap_q)
    hr, wr = U.grid((Hr, Wr), P, wrap_r)
    idx = np.asarray(idx).reshape(h, w).astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    total = np.zeros((3, H, W), np.float32)
    cnt = np.zeros((H, W), np.int64)
    for dy in range(P):
        for dx in range(P):
            py, px = ys - dy, xs - dx
            if wrap_q[0]:
                py = py % H
            if wrap_q[1]:
                px = px % W
            on = (py >= 0) & (py < h) & (px >= 0) & (px < w)
            n = np.where(on, idx[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)], -1)
            on &= (n >= 0) & (n < hr * wr)
            n = np.where(on, n, 0)
            yy, xx = (n // wr + dy) % Hr, (n % wr + dx) % Wr
            val = ref[:, yy, xx]
            total = np.where(on[None], (total + val).astype(np.float32), total)
            cnt += on
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (total / cnt.astype(np.float32)[None]).astype(np.float32)
    g = np.full((H, W), np.float32(blend)) if weight is None else (np.float32(blend) * np.asarray(weight, np.float32))
    g = np.broadcast_to(g.astype(np.float32)[None], base.shape)
    keep = (g == 0) | np.broadcast_to(cnt[None] == 0, base.shape)
    with np.errstate(invalid="ignore"):
        mixed = ((g * (mean - base).astype(np.float32)).astype(np.float32) + base).astype(np.float32)
    return np.where(keep, base, np.where(g == 1, mean, mixed)).astype(np.float32)


# ---- the field and the loop, float64 ----

def field64(x, ref, P, wrap_q=(False, False), wrap_r=(False, False), ok=None, scale=None):
    """Brute force: (idx (M,), D (M, N) with +inf where not admissible).  `scale` (N,): the winner minimises D * scale."""
    A, _ = U.patches(x, P, wrap_q)
    Bm, _ = U.patches(ref, P, wrap_r)
    D = U.distances(A, Bm)
    if ok is not None:
        D[:, ~np.asarray(ok).reshape(-1).astype(bool)] = np.inf
    V = D if scale is None else D * np.asarray(scale, np.float64).reshape(1, -1)
    return V.argmin(axis=1), D


def energy64(x, ref, P, wrap_q=(False, False), ok=None):
    """E*(x) = sum_i min_j |P_i x - b_j|^2, float64, and tau_i summed (nnf_util.check_field's tau)."""
    A, _ = U.patches(x, P, wrap_q)
    idx, D = field64(x, ref, P, wrap_q, ok=ok)
    return float(D.min(axis=1).sum()), float(tau(A, U.patches(ref, P)[0], P, ok).sum())


def tau(A, Bm, P, ok=None):
    """tau_i of nnf_util.check_field: the forward error of two fp32 ranking chains."""
    K = 3 * P * P
    kpad = (K + 3) // 4 * 4
    adm = np.ones(Bm.shape[0], bool) if ok is None else np.asarray(ok).reshape(-1).astype(bool)
    nb = np.einsum("nk,nk->n", Bm[adm], Bm[adm]).max()
    na = np.sqrt(np.einsum("mk,mk->m", A, A))
    return 2.0 * (kpad + 3) * U24 * (nb + 2.0 * na * np.sqrt(nb))


def vote64(idx, ref, base, P, wrap_q=(False, False), blend=1.0):
    """The vote in float64 (no reference wrap): the loop's second half."""
    ref, base = np.asarray(ref, np.float64), np.asarray(base, np.float64)
    _, H, W = base.shape
    h, w = U.grid((H, W), P, wrap_q)
    wr = ref.shape[2] - P + 1
    idx = np.asarray(idx).reshape(h, w)
    total, cnt = np.zeros_like(base), np.zeros((H, W))
    for py in range(h):
        for px in range(w):
            ry, rx = divmod(int(idx[py, px]), wr)
            yy = (py + np.arange(P)) % H
            xx = (px + np.arange(P)) % W
            total[:, yy[:, None], xx[None]] += ref[:, ry:ry + P, rx:rx + P]
            cnt[yy[:, None], xx[None]] += 1
    return base + blend * (total / cnt - base)


def refine64(x, ref, P, iters, wrap_q=(False, False), blend=1.0, alpha=None):
    """The loop in float64: ([E*(x_0), ..., E*(x_iters)], x_iters, the first iteration's winners)."""
    K = 3 * P * P
    es, first = [], None
    for _ in range(iters):
        scale = None
        if alpha is not None:
            _, back = field64(ref, x, P, wrap_r=wrap_q)
            scale = 1.0 / (alpha * K + back.min(axis=1))
        idx, D = field64(x, ref, P, wrap_q, scale=scale)
        first = idx if first is None else first
        es.append(float(D.min(axis=1).sum()))
        x = vote64(idx, ref, x, P, wrap_q, blend)
    es.append(energy64(x, ref, P, wrap_q)[0])
    return es, x, first


def completeness_scale(x, ref, P, wrap_q=(False, False), alpha=ALPHA):
    """s_j = 1 / (alpha 3 P^2 + min_i D_ij) as float32 (hr, wr): what patch_refine hands the scaled search."""
    _, back = field64(ref, x, P, wrap_r=wrap_q)
    s = 1.0 / (alpha * 3 * P * P + back.min(axis=1))
    return s.astype(np.float32).reshape(U.grid(np.asarray(ref).shape[1:], P, (False, False)))


# ---- the scaled ranking: float32 emulation of the contract and the bound against float64 ----

def _fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def scaled_values_f32(A, Bm, scale):
    """v of sinddm_patch_nnf_scaled for every pair, (M, N) float32: |b|^2 and |a|^2 as fmaf chains over k from 0, r continued
    from |b|^2 with -2 a_k b_k, t = r + |a|^2 (one add), v = max(t, 0) * s (one multiply).  (Every product of two float32
    is exact in float64; the sum is rounded to float64 and then to float32, which differs from a true fmaf only in rare
    double roundings -- this emulation is held to the bound, not to bits.)"""
    A, Bm = np.asarray(A, np.float32), np.asarray(Bm, np.float32)
    M, N, K = A.shape[0], Bm.shape[0], A.shape[1]
    nb, na = np.zeros(N, np.float32), np.zeros(M, np.float32)
    for k in range(K):
        nb = _fmaf(Bm[:, k], Bm[:, k], nb)
        na = _fmaf(A[:, k], A[:, k], na)
    r = np.broadcast_to(nb[None], (M, N)).astype(np.float32)
    m2a = (np.float32(-2.0) * A).astype(np.float32)
    for k in range(K):
        r = _fmaf(np.broadcast_to(m2a[:, k:k + 1], (M, N)), np.broadcast_to(Bm[None, :, k], (M, N)), r)
    t = (r + na[:, None]).astype(np.float32)
    return (np.maximum(t, np.float32(0)) * np.asarray(scale, np.float32).reshape(1, -1)).astype(np.float32)


def scaled_values_64(query, ref, P, scale, wrap_q=(False, False), wrap_r=(False, False)):
    """(v64 (M, N) = D_ij s_j, e (M, N) = the bound of check_scaled_field for every pair), no admissibility."""
    A, _ = U.patches(query, P, wrap_q)
    Bm, _ = U.patches(ref, P, wrap_r)
    s = np.asarray(scale, np.float64).reshape(1, -1)
    D = U.distances(A, Bm)
    na = np.einsum("mk,mk->m", A, A)
    e = s * (tau(A, Bm, P)[:, None] / 2.0 + (3 * P * P + 3) * U24 * (na[:, None] + D))
    return D * s, e


def check_scaled_field(query, ref, P, scale, idx, dist=None, wrap_q=(False, False), wrap_r=(False, False), ok=None, what=""):
    """The criteria of the scaled field of ONE sample against float64 brute force of v64_ij = D_ij s_j:
      every winner admissible;
      v64(i, sel) - min_j v64(i, j) <= e(i, sel) + e(i, argmin),
          e_ij = s_j (tau_i / 2 + (3 P^2 + 3) 2^-24 (|a_i|^2 + D_ij));
      |dist - D(i, sel)| <= (K + 4) 2^-24 D(i, sel)  (when `dist` is given).
    Where e comes from (u = 2^-24, K = 3 P^2): the computed ranking value is v^ = fl(max(t^, 0) s_j) with t^ = fl(r^ + na^).
    r^ = r + d_r with |d_r| <= tau_i / 2 -- tau_i is check_field's bound for the difference of TWO ranking chains, so half of
    it bounds one.  na^ is a chain of K fmafs of non-negative terms: na^ = |a_i|^2 (1 + th), |th| <= K u / (1 - K u).  The
    exact t = r + |a_i|^2 is D_ij >= 0, so t^ = (D_ij + d_r + |a_i|^2 th)(1 + e1); clamping at 0 moves t^ towards D_ij and adds
    nothing; the multiply adds (1 + e2).  To first order |v^ - D_ij s_j| <= s_j (|d_r| + K u |a_i|^2 + 2 u D_ij), and the
    three further u on each of |a_i|^2 and D_ij (and the K_pad + 3 steps tau allows a chain of K_pad + 1 roundings) cover
    the second-order terms at K u <= 147 * 6e-8.  The search takes the smallest v^ (ties change nothing: equal v^), so
    v64(sel) - e(sel) <= v^(sel) <= v^(argmin) <= v64(argmin) + e(argmin).
    Returns the worst ratio gap / (e_sel + e_min)."""
    A, _ = U.patches(query, P, wrap_q)
    Bm, _ = U.patches(ref, P, wrap_r)
    M, N, K = A.shape[0], Bm.shape[0], 3 * P * P
    s = np.asarray(scale, np.float64).reshape(-1)
    idx = np.asarray(idx).reshape(-1).astype(np.int64)
    assert s.shape == (N,) and idx.shape == (M,), (what, s.shape, N, idx.shape, M)
    assert idx.min() >= 0 and idx.max() < N, (what, idx.min(), idx.max())
    adm = np.ones(N, bool) if ok is None else np.asarray(ok).reshape(-1).astype(bool)
    assert adm[idx].all(), f"{what}: {int((~adm[idx]).sum())} winners are not admissible"
    D = U.distances(A, Bm)
    D[:, ~adm] = np.inf
    V = D * s[None]
    jmin = V.argmin(axis=1)
    rows = np.arange(M)
    na = np.einsum("mk,mk->m", A, A)
    t = tau(A, Bm, P, ok)

    def e(j):
        return s[j] * (t / 2.0 + (K + 3) * U24 * (na + D[rows, j]))

    gap = V[rows, idx] - V[rows, jmin]
    bound = e(idx) + e(jmin)
    ratio = float((gap / bound).max())
    msg = f"{what}: M {M} N {N} max gap {gap.max():.3e} worst gap / bound {ratio:.3f} index mismatches {int((idx != jmin).sum())}"
    if dist is not None:
        dsel = D[rows, idx]
        derr = np.abs(np.asarray(dist, np.float64).reshape(-1) - dsel)
        dbound = (K + 4) * U24 * dsel
        msg += f" worst dist ratio {(derr / np.maximum(dbound, 1e-300)).max():.3f}"
    print(msg)
    assert (gap <= bound).all(), f"{what}: {int((gap > bound).sum())} queries beyond the bound, worst ratio {ratio:.3f}"
    if dist is not None:
        assert (derr <= dbound).all(), f"{what}: {int((derr > dbound).sum())} distances beyond the bound"
    return ratio
