"""Numpy twin of rp_actor_step (include/learn/rp_actor.h), statement by statement: the policy, every critic at the policy's
action, the selection of the minimum, the head gradient, the actor's backward pass, the parameter gradients, Adam on the
actor and on log_alpha, and the five statistics.

The noise and the dropout masks are integer arithmetic on the planner's Philox twin with the step's own counter words
(64 + j and 80 + 2 i + L): the kernel's bit for bit.  Everything else is the header's formulae in a dtype of the caller's
choice: float64 is the reference, float32 the restatement whose own error against float64 sets the bar of the kernel's.
The sums follow the header's order through critic_reference's routines (the LayerNorm sums and a critic's head: sixteen
lanes, then a tree; the batch sums: the rows of a tile of 16 ascending, then the tiles ascending; M: MSUM; the products: a
fused-multiply-add chain over the reduction index ascending, in float32 -- the float64 reference uses numpy's product).
`permute` gives a second restatement whose k order, unit order, action order and batch-row order are shuffled.  Scalars
are cast to the dtype as given: a caller who wants the kernel's float32 constants in the float64 reference passes them
rounded.
"""

from __future__ import annotations

import numpy as np

import critic_reference as cr
import droq_reference as dr
import learn_reference as lr
import plan_reference as pr

NOISE_COUNTER = 64
COUNTER = 80
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")
STATS = ("actor_loss", "alpha_loss", "alpha", "entropy", "masked")
ADAM = ("step_size", "bc2_sqrt", "eps", "omb1", "beta2", "omb2")
LN_2, LN_2PI = 0.6931471805599453, 1.8378770664093453


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def noise(seed, round_, rows, A):
    """za(seed, round, b, u) for the absolute batch rows `rows` and u < A, float64 [len(rows), A]: plan_reference.z with
    the last counter word moved by NOISE_COUNTER."""
    e, c = np.asarray(rows, np.uint64)[:, None], np.arange(A, dtype=np.uint64)[None, :]
    S = np.zeros((len(rows), A), np.uint64)
    for j in range(3):
        for w in pr.philox4x32_10((round_, e, c, NOISE_COUNTER + j), _key(seed)):
            S = S + w
    return (S.astype(np.int64) - (np.int64(6) << np.int64(32))).astype(np.float64) * 2.0 ** -32


def masks(rows, H, critic, layer, seed, round_, threshold):
    """droq_reference.masks with the actor step's counter."""
    rows = np.asarray(rows, np.uint64)
    grp = np.arange(H // 4, dtype=np.uint64)
    w = pr.philox4x32_10((round_, rows[:, None], grp[None, :], COUNTER + 2 * critic + layer), _key(seed))
    return np.stack(w, axis=-1).reshape(len(rows), H) >= np.uint64(threshold)


def _chain(x, order=None):
    """The sum over the last axis of x [rows, n], one chain from 0, ascending or in `order`."""
    s = np.zeros(x.shape[0], x.dtype.type)
    for u in (range(x.shape[1]) if order is None else order):
        s = s + x[:, u]
    return s


def adam(p, m, v, g, step_size, bc2_sqrt, eps, omb1, beta2, omb2):
    """rp_critic.h's ADAM statements without the Polyak step; returns (p, m, v)."""
    return cr.adam(p, m, v, p, g, step_size, bc2_sqrt, eps, omb1, beta2, omb2, p.dtype.type(0))[:3]


def step(obs, mask, mean, inv_std, clip, actor, m, v, critics, log_alpha, log_alpha_m, log_alpha_v, target_entropy,
         log_std_bounds, *, actor_adam, alpha_adam, threshold=0, keep_scale=1.0, ln_eps=1e-5, seed=0, round_=0,
         dtype=np.float64, row_first=0, row_count=None, permute=None):
    """actor, m, v: the six arrays in PARAMS' order; critics: a sequence of the ten arrays in critic_reference.PARAMS'
    order; actor_adam, alpha_adam: dicts of ADAM's keys.  -> {"action" [row_count, A], "logp", "q_min" [row_count], "grad",
    "p", "m", "v": six arrays each, "log_alpha": {"grad", "p", "m", "v"} (arrays of one element), "stats" [5], and what
    the twin chose: "best" (the selected critic per row), "inside" [row_count, A], "noise" (zf), "masks" (per critic: keep of
    layer 1, of layer 2), "q" [n_critics, row_count], "head_l" (l before the clamp)}; row r is batch row row_first + r.
    `permute`: a seed; every summation order is then shuffled."""
    t = dtype
    n = len(obs)
    row_count = n - row_first if row_count is None else row_count
    rows = np.arange(row_first, row_first + row_count)
    rng = np.random.default_rng(permute) if permute is not None else None
    border = rng.permutation(row_count) if rng is not None else None
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, t) for a in actor)
    A, D = len(b3) // 2, w1.shape[1]
    xn = lr.normalize(np.asarray(obs)[rows], mean, inv_std, clip, t)
    mk = np.asarray(mask, t)[rows]
    M = np.fmax(cr.mask_sum(mk), t(1))
    w = mk / M
    la0 = np.asarray(log_alpha, t).reshape(1)
    al = np.exp(la0)[0]
    ks, le, te = t(keep_scale), t(ln_eps), t(target_entropy)
    lo, hi = t(log_std_bounds[0]), t(log_std_bounds[1])
    const = (lambda x: t(np.float32(x))) if t is np.float32 else t
    # 1. the policy
    h1 = np.tanh(cr._matmul(xn, w1, rng) + b1)
    h2 = np.tanh(cr._matmul(h1, w2, rng) + b2)
    head = cr._matmul(h2, w3, rng) + b3
    mu, l = head[:, :A], head[:, A:]
    ls = np.fmin(np.fmax(l, lo), hi)
    inside = (l > lo) & (l < hi)
    zf = noise(seed, round_, rows, A).astype(np.float32).astype(t)
    sd = np.exp(ls)
    tt = sd * zf
    p = mu + tt
    a = np.tanh(p)
    ww = t(-2) * p
    sp = np.fmax(ww, t(0)) + np.log1p(np.exp(-np.abs(ww)))
    lg = t(2) * ((const(LN_2) - p) - sp)
    term = (t(-0.5) * (zf * zf) - ls) - lg
    logp = _chain(term, rng.permutation(A) if rng is not None else None) - const(0.5 * A * LN_2PI)
    # 2. the critics and the selection
    x = np.concatenate([xn, a], axis=1)
    qm, best, dqa = None, np.zeros(row_count, np.int64), np.zeros((row_count, A), t)
    qs, kept = [], []
    for i, net in enumerate(critics):
        cw1, cb1, cw2, cb2, cw3, cb3, g1, be1, g2, be2 = (np.asarray(c_, t) for c_ in net)
        k1 = masks(rows, len(cb1), i, 0, seed, round_, threshold)
        k2 = masks(rows, len(cb2), i, 1, seed, round_, threshold)
        out1, o1, r1 = cr._forward(x, cw1, cb1, g1, be1, k1, ks, le, t, rng)
        out2, o2, r2 = cr._forward(out1, cw2, cb2, g2, be2, k2, ks, le, t, rng)
        horder = rng.permutation(len(cb2)) if rng is not None else None
        q = dr.row_sum(out2 * cw3[0], horder) + cb3[0]
        # BACKWARD with dq = 1, then the A action columns of W1
        _, ds2 = cr._backward(np.broadcast_to(cw3[0], out2.shape), out2, o2, r2, g2, k2, ks, t, rng)
        dout1 = cr._matmul(ds2, np.ascontiguousarray(cw2.T), rng)
        _, ds1 = cr._backward(dout1, out1, o1, r1, g1, k1, ks, t, rng)
        dq_a = cr._matmul(ds1, np.ascontiguousarray(cw1[:, D:].T), rng)
        take = np.ones(row_count, bool) if i == 0 else q < qm
        qm = np.where(take, q, qm) if i else q
        best = np.where(take, i, best)
        dqa = np.where(take[:, None], dq_a, dqa)
        qs.append(q)
        kept.append((k1, k2))
    # 3. the loss's terms and the head gradient
    s1 = al * logp
    la = w * (s1 - qm)
    gt = w * (logp + te)
    en = w * logp
    wa = (al * w)[:, None]
    e2 = wa * (t(2) * a)
    om = t(1) - a * a
    f2 = (w[:, None] * dqa) * om
    dp = e2 - f2
    dl = np.where(inside, dp * tt - wa, t(0))
    dout3 = np.concatenate([dp, dl], axis=1)
    # 4. the actor's backward pass and the parameter gradients
    dh2 = cr._matmul(dout3, np.ascontiguousarray(w3.T), rng)
    ds2 = dh2 * (t(1) - h2 * h2)
    dh1 = cr._matmul(ds2, np.ascontiguousarray(w2.T), rng)
    ds1 = dh1 * (t(1) - h1 * h1)
    T = lambda z: np.ascontiguousarray(z.T)
    grads = [cr._matmul(T(ds1), T(xn), rng), cr.tile_sum(ds1, border), cr._matmul(T(ds2), T(h1), rng), cr.tile_sum(ds2, border),
             cr._matmul(T(dout3), T(h2), rng), cr.tile_sum(dout3, border)]
    sc = [t(actor_adam[k]) for k in ADAM]
    new = [adam(np.asarray(p_, t), np.asarray(m_, t), np.asarray(v_, t), g_, *sc) for p_, m_, v_, g_ in zip(actor, m, v, grads)]
    # 5. the temperature
    g = -cr.tile_sum(gt, border).reshape(1)
    sc = [t(alpha_adam[k]) for k in ADAM]
    la1, lam, lav = adam(la0, np.asarray(log_alpha_m, t).reshape(1), np.asarray(log_alpha_v, t).reshape(1), g, *sc)
    # 6. the statistics
    stats = np.array([cr.tile_sum(la, border), la0[0] * g[0], np.exp(la1[0]), -cr.tile_sum(en, border),
                      t(1) - cr.tile_sum(mk, border) / t(row_count)], t)
    return {"action": a, "logp": logp, "q_min": qm, "grad": grads, "p": [x_[0] for x_ in new], "m": [x_[1] for x_ in new],
            "v": [x_[2] for x_ in new], "log_alpha": {"grad": g, "p": la1, "m": lam, "v": lav}, "stats": stats,
            "best": best, "inside": inside, "noise": zf, "masks": kept, "q": np.stack(qs), "head_l": l}
