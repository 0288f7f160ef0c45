"""Numpy twin of rp_droq_target (include/learn/rp_droq.h), line by line.

The dropout masks are integer arithmetic on the planner's Philox twin (plan_reference.philox4x32_10): they are the
kernel's bit for bit.  Everything else is the header's formulae in a dtype of the caller's choice: float64 is the
reference, float32 the restatement whose own error against float64 sets the bar of the kernel's.  The two sums of the
LayerNorm are taken in the header's order (sixteen lanes, then a balanced tree); `permute` gives a second restatement
whose k order and unit order are shuffled, which is how the host tests measure the conditioning of a case.  The
normaliser is the learner's twin (learn_reference), the TD epilogue sac_reference.target's.
"""

from __future__ import annotations

import numpy as np

import learn_reference as lr
import plan_reference as pr

COUNTER = 32
LANES = 16


def drop_threshold(p):
    return min(int(p * 2 ** 32), 2 ** 32 - 1)


def masks(rows, H, critic, layer, seed, round_, threshold):
    """keep [len(rows), H] (bool) of hidden layer `layer` in {0, 1} of critic `critic` for the absolute batch rows `rows`."""
    rows = np.asarray(rows, np.uint64)
    grp = np.arange(H // 4, dtype=np.uint64)
    w = pr.philox4x32_10((round_, rows[:, None], grp[None, :], COUNTER + 2 * critic + layer),
                         (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    words = np.stack(w, axis=-1).reshape(len(rows), H)       # unit n: word n & 3 of group n >> 2
    return words >= np.uint64(threshold)


def lane_units(H):
    """The units of lane j, in the order the lane adds them: the groups j, j + 16, ... ascending, four units each."""
    return [[4 * g + c for g in range(j, H // 4, LANES) for c in range(4)] for j in range(LANES)]


def row_sum(x, order=None):
    """SUM of the header over the last axis of x [rows, H]: the lanes' partial sums from 0, then p[j] + p[j ^ m] for
    m = 1, 2, 4, 8.  With `order` (a permutation of the units): one chain from 0 in that order instead."""
    t = x.dtype.type
    if order is not None:
        s = np.zeros(x.shape[0], t)
        for n in order:
            s = s + x[:, n]
        return s
    p = np.zeros((x.shape[0], LANES), t)
    for j, units in enumerate(lane_units(x.shape[1])):
        for n in units:
            p[:, j] = p[:, j] + x[:, n]
    lanes = np.arange(LANES)
    for m in (1, 2, 4, 8):
        p = p + p[:, lanes ^ m]
    return p[:, 0]


def hidden(x, W, bb, g, be, keep, keep_scale, ln_eps, dtype, rng=None):
    """One hidden layer: Linear -> dropout (the mask `keep`) -> LayerNorm -> ReLU."""
    t = dtype
    W, x = np.asarray(W, t), np.asarray(x, t)
    if rng is not None:
        k = rng.permutation(W.shape[1])
        x, W = np.ascontiguousarray(x[:, k]), np.ascontiguousarray(W[:, k])
    H = W.shape[0]
    s = x @ W.T + np.asarray(bb, t)
    h = np.where(keep, s * t(np.float32(keep_scale)), t(0))
    order = rng.permutation(H) if rng is not None else None
    mu = row_sum(h, order) / t(H)
    d = h - mu[:, None]
    var = row_sum(d * d, order) / t(H)
    r = t(1) / np.sqrt(var + t(np.float32(ln_eps)))
    o = d * r[:, None]
    o = o * np.asarray(g, t)
    o = o + np.asarray(be, t)
    return np.fmax(o, t(0))


def target(next_obs, action, logp, reward, discount, mean, inv_std, clip, gamma, log_alpha, critics, threshold=0,
           keep_scale=1.0, ln_eps=1e-5, seed=0, round_=0, dtype=np.float64, row_first=0, row_count=None, permute=None):
    """critics: a sequence of (w1, b1, w2, b2, w3, b3, g1, be1, g2, be2).  -> {"y", "q_min" [row_count], "q"
    [n_critics, row_count], "masks": per critic (keep of layer 1, keep of layer 2)} for the rows of the range (row r of
    the output is batch row row_first + r).  `permute`: a seed; the k order of every product and the unit order of every
    LayerNorm sum are then shuffled (a restatement in another order, not the kernel's)."""
    t = dtype
    n = len(next_obs)
    row_count = n - row_first if row_count is None else row_count
    rows = np.arange(row_first, row_first + row_count)
    rng = np.random.default_rng(permute) if permute is not None else None
    xa = np.concatenate([lr.normalize(np.asarray(next_obs)[rows], mean, inv_std, clip, t),
                         np.asarray(action, t)[rows]], axis=1)
    qs, kept = [], []
    for i, (w1, b1, w2, b2, w3, b3, g1, be1, g2, be2) in enumerate(critics):   # (ascending, as the kernel)
        m1 = masks(rows, len(b1), i, 0, seed, round_, threshold)
        m2 = masks(rows, len(b2), i, 1, seed, round_, threshold)
        h1 = hidden(xa, w1, b1, g1, be1, m1, keep_scale, ln_eps, t, rng)
        h2 = hidden(h1, w2, b2, g2, be2, m2, keep_scale, ln_eps, t, rng)
        w3 = np.asarray(w3, t)
        if rng is not None:
            k = rng.permutation(w3.shape[1])
            h2, w3 = np.ascontiguousarray(h2[:, k]), np.ascontiguousarray(w3[:, k])
        qs.append((h2 @ w3.T + np.asarray(b3, t))[:, 0])
        kept.append((m1, m2))
    qm = qs[0]
    for q in qs[1:]:
        qm = np.fmin(qm, q)
    al = np.exp(t(np.float32(log_alpha)))
    s = al * np.asarray(logp, t)[rows]
    v = qm - s
    nv = t(np.float32(gamma)) * np.asarray(discount, t)[rows]
    tv = nv * v
    return {"y": np.asarray(reward, t)[rows] + tv, "q_min": qm, "q": np.stack(qs), "masks": kept}
