"""Float64 numpy brute force of the patch nearest-neighbour field: the reference of the sinddm_patch_nnf tests (test code,
not product code).  Patch element order (c, dy, dx), positions row-major, wrapped axes by np.concatenate."""
import numpy as np


def grid(size, P, wrap):
    return tuple(int(n) if w else int(n) - P + 1 for n, w in zip(size, wrap))


def patches(img, P, wrap=(False, False)):
    """(3, H, W) -> ((h w, 3 P^2) float64 patch matrix, (h, w))."""
    img = np.asarray(img, dtype=np.float64)
    if wrap[0]:
        img = np.concatenate([img, img[:, :P - 1]], axis=1)
    if wrap[1]:
        img = np.concatenate([img, img[:, :, :P - 1]], axis=2)
    v = np.lib.stride_tricks.sliding_window_view(img, (P, P), axis=(1, 2))          # (3, h, w, P, P)
    h, w = v.shape[1], v.shape[2]
    return np.ascontiguousarray(v.transpose(1, 2, 0, 3, 4)).reshape(h * w, 3 * P * P), (h, w)


def position_ok(valid, P, wrap=(False, False)):
    """(H, W) pixel map -> (h w,) bool: all P x P pixels of the patch are valid."""
    v = np.asarray(valid, dtype=np.float64)
    if wrap[0]:
        v = np.concatenate([v, v[:P - 1]], axis=0)
    if wrap[1]:
        v = np.concatenate([v, v[:, :P - 1]], axis=1)
    return np.lib.stride_tricks.sliding_window_view(v, (P, P)).min(axis=(2, 3)).reshape(-1) > 0


def distances(A, Bm):
    """All squared distances (M, N), float64, row by row as differences (no cancellation)."""
    out = np.empty((A.shape[0], Bm.shape[0]))
    for i in range(A.shape[0]):
        d = Bm - A[i]
        out[i] = np.einsum("nk,nk->n", d, d)
    return out


def check_field(query, ref, P, idx, dist, wrap_q=(False, False), wrap_r=(False, False), ok=None, what=""):
    """The two criteria every query must meet, against brute force over the admissible set:
      gap   d64(q, idx) - min_j d64(q, j) <= tau(q) = 2 (K_pad + 3) 2^-24 (max |b|^2 + 2 |a| max |b|): the forward error of
            two fp32 ranking chains r = |b|^2 - 2 a.b
      dist  |dist - d64(q, idx)| <= (K + 4) 2^-24 d64(q, idx)
    `idx` / `dist` are the field of ONE sample, any shape with h w entries.  Returns (worst gap / tau, worst dist ratio)."""
    A, _ = patches(query, P, wrap_q)
    Bm, _ = patches(ref, P, wrap_r)
    idx = np.asarray(idx).reshape(-1).astype(np.int64)
    dist = np.asarray(dist, dtype=np.float64).reshape(-1)
    M, N = A.shape[0], Bm.shape[0]
    assert idx.shape == (M,) and dist.shape == (M,), (what, idx.shape, M)
    assert idx.min() >= 0 and idx.max() < N, (what, idx.min(), idx.max(), N)
    adm = np.ones(N, bool) if ok is None else np.asarray(ok).reshape(-1).astype(bool)
    assert adm[idx].all(), f"{what}: {int((~adm[idx]).sum())} winners are not admissible"
    D = distances(A, Bm)
    D[:, ~adm] = np.inf
    dmin = D.min(axis=1)
    dsel = D[np.arange(M), idx]
    K = 3 * P * P
    kpad = (K + 3) // 4 * 4
    nb = np.einsum("nk,nk->n", Bm[adm], Bm[adm]).max()
    na = np.sqrt(np.einsum("mk,mk->m", A, A))
    tau = 2.0 * (kpad + 3) * 2.0 ** -24 * (nb + 2.0 * na * np.sqrt(nb))
    gap = dsel - dmin
    derr = np.abs(dist - dsel)
    dbound = (K + 4) * 2.0 ** -24 * dsel
    print(f"{what}: M {M} N {N} admissible {int(adm.sum())} max gap {gap.max():.3e} (tau max {tau.max():.3e}, median nearest "
          f"{np.median(dmin):.3e}) max |dist - d64| {derr.max():.3e} worst dist ratio "
          f"{(derr / np.maximum(dbound, 1e-300)).max():.3f} index mismatches {int((idx != D.argmin(axis=1)).sum())}")
    assert (gap <= tau).all(), f"{what}: {int((gap > tau).sum())} queries beyond tau, worst {gap.max():.3e}"
    assert (derr <= dbound).all(), f"{what}: {int((derr > dbound).sum())} distances beyond the bound, worst {derr.max():.3e}"
    return float((gap / tau).max()), float((derr / np.maximum(dbound, 1e-300)).max())
