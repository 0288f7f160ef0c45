"""Numpy twin of rp_critic_step (include/learn/rp_critic.h), line by line: the forward pass of every critic, the loss
gradient, the row-local backward pass, the parameter gradients, Adam and the Polyak step.

The dropout masks are droq_reference's Philox with the critic step's counter (48 + 2 i + L): integers, the kernel's bit
for bit.  Everything else is the header's formulae in a dtype of the caller's choice: float64 is the reference, float32
the restatement whose own error against float64 sets the bar of the kernel's.  The sums follow the header's order (the
LayerNorm sums and the head: sixteen lanes, then a balanced tree; the vector gradients: the rows of a tile of 16 ascending,
then the tiles ascending; M: 256 strided chains, then a tree; the products: a fused-multiply-add chain over the reduction
index ascending, in float32 -- the float64 reference uses numpy's product).  `permute` gives a second
restatement whose k order, unit order and batch-row order are shuffled, which is how the host tests measure the
conditioning of a case.  Scalars are cast to the dtype as given: a caller who wants the kernel's float32 constants in the
float64 reference passes them rounded.
"""

from __future__ import annotations

import numpy as np

import droq_reference as dr
import learn_reference as lr
import plan_reference as pr

COUNTER = 48
TILE = 16
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3", "g1", "be1", "g2", "be2")


def masks(rows, H, critic, layer, seed, round_, threshold):
    """droq_reference.masks with the live critics' counter."""
    rows = np.asarray(rows, np.uint64)
    grp = np.arange(H // 4, dtype=np.uint64)
    w = pr.philox4x32_10((round_, rows[:, None], grp[None, :], COUNTER + 2 * critic + layer),
                         (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.stack(w, axis=-1).reshape(len(rows), H) >= np.uint64(threshold)


def mask_sum(mask):
    """MSUM of the header: thread t of 256 adds mask[t + 256 j], j ascending; then p[t] + p[t + 128], + 64, .. + 1."""
    t = mask.dtype.type
    n = -(-len(mask) // 256) * 256
    x = np.zeros(n, t)
    x[:len(mask)] = mask
    p = np.zeros(256, t)
    for row in x.reshape(-1, 256):
        p = p + row
    s = 128
    while s:
        p = p[:s] + p[s:2 * s]
        s >>= 1
    return p[0]


def tile_sum(x, order=None):
    """The batch sum of x [R, ...]: tiles of 16 rows, rows ascending from 0, then tiles ascending from 0.  With `order`
    (a permutation of the rows): one chain from 0 in that order."""
    t = x.dtype.type
    if order is not None:
        s = np.zeros(x.shape[1:], t)
        for b in order:
            s = s + x[b]
        return s
    total = np.zeros(x.shape[1:], t)
    for l0 in range(0, len(x), TILE):
        s = np.zeros(x.shape[1:], t)
        for row in x[l0:l0 + TILE]:
            s = s + row
        total = total + s
    return total


def _matmul(x, W, rng):
    """x W^T.  float32: the header's fused-multiply-add chain over the reduction index ascending, from 0 (a product of two
    float32 is exact in float64, so each link is rounded once to float64 and once to float32: a fused multiply-add but
    for rare double roundings).  float64 (the reference): numpy's product.  With rng (the restatement in another order):
    numpy's product on a shuffled reduction index."""
    if rng is not None:
        k = rng.permutation(W.shape[1])
        x, W = np.ascontiguousarray(x[:, k]), np.ascontiguousarray(W[:, k])
        return x @ W.T
    if x.dtype != np.float32:
        return x @ W.T
    x64, w64 = x.astype(np.float64), W.astype(np.float64)
    acc = np.zeros((x.shape[0], W.shape[0]), np.float32)
    for k in range(W.shape[1]):
        acc = (acc.astype(np.float64) + x64[:, k, None] * w64[None, :, k]).astype(np.float32)
    return acc


def _forward(x, W, bb, g, be, keep, ks, eps, t, rng):
    H = W.shape[0]
    s = _matmul(x, W, rng) + bb
    h = np.where(keep, s * ks, t(0))
    order = rng.permutation(H) if rng is not None else None
    mu = dr.row_sum(h, order) / t(H)
    d = h - mu[:, None]
    var = dr.row_sum(d * d, order) / t(H)
    r = t(1) / np.sqrt(var + eps)
    o = d * r[:, None]
    u = o * g
    u = u + be
    return np.fmax(u, t(0)), o, r


def _backward(dout, out, o, r, g, keep, ks, t, rng):
    H = out.shape[1]
    dz = np.where(out > 0, dout, t(0))
    c = dz * g
    order = rng.permutation(H) if rng is not None else None
    m1 = dr.row_sum(c, order) / t(H)
    m2 = dr.row_sum(c * o, order) / t(H)
    t1 = c - m1[:, None]
    t2 = o * m2[:, None]
    t3 = t1 - t2
    dh = r[:, None] * t3
    return dz, np.where(keep, dh * ks, t(0))


def adam(p, m, v, tg, g, step_size, bc2_sqrt, eps, omb1, beta2, omb2, tau):
    """The header's statements on arrays of one dtype; returns (p, m, v, target)."""
    a = g - m
    a = a * omb1
    m = m + a
    c = g * omb2
    c = c * g
    v = v * beta2
    v = v + c
    den = np.sqrt(v) / bc2_sqrt
    den = den + eps
    u = m / den
    u = u * step_size
    p = p - u
    w = p - tg
    w = w * tau
    return p, m, v, tg + w


def step(obs, action, y, mask, mean, inv_std, clip, critics, m, v, targets, *, step_size, bc2_sqrt, eps=1e-8, omb1=0.1,
         beta2=0.999, omb2=0.001, tau=0.005, threshold=0, keep_scale=1.0, ln_eps=1e-5, seed=0, round_=0, dtype=np.float64,
         row_first=0, row_count=None, permute=None):
    """critics, m, v, targets: a sequence (per critic) of the ten arrays in PARAMS' order.  -> {"q" [n_critics, row_count],
    "grad", "p", "m", "v", "target": per critic a list of ten arrays, "masks": per critic (keep of layer 1, of layer 2)};
    row r of q is batch row row_first + r.  `permute`: a seed; every summation order is then shuffled."""
    t = dtype
    n = len(obs)
    row_count = n - row_first if row_count is None else row_count
    rows = np.arange(row_first, row_first + row_count)
    rng = np.random.default_rng(permute) if permute is not None else None
    x = np.concatenate([lr.normalize(np.asarray(obs)[rows], mean, inv_std, clip, t), np.asarray(action, t)[rows]], axis=1)
    yy, mk = np.asarray(y, t)[rows], np.asarray(mask, t)[rows]
    M = np.fmax(mask_sum(mk), t(1))
    ks, le = t(keep_scale), t(ln_eps)
    sc = [t(s) for s in (step_size, bc2_sqrt, eps, omb1, beta2, omb2, tau)]
    out = {k: [] for k in ("q", "grad", "p", "m", "v", "target", "masks")}
    for i, net in enumerate(critics):
        w1, b1, w2, b2, w3, b3, g1, be1, g2, be2 = (np.asarray(a, t) for a in net)
        k1 = masks(rows, len(b1), i, 0, seed, round_, threshold)
        k2 = masks(rows, len(b2), i, 1, seed, round_, threshold)
        out1, o1, r1 = _forward(x, w1, b1, g1, be1, k1, ks, le, t, rng)
        out2, o2, r2 = _forward(out1, w2, b2, g2, be2, k2, ks, le, t, rng)
        horder = rng.permutation(len(b2)) if rng is not None else None
        q = dr.row_sum(out2 * w3[0], horder) + b3[0]
        e = q - yy
        f = mk * e
        dq = f / M
        border = rng.permutation(row_count) if rng is not None else None
        dw3 = tile_sum(dq[:, None] * out2, border)[None, :]
        db3 = tile_sum(dq, border).reshape(1)
        dz2, ds2 = _backward(dq[:, None] * w3[0][None, :], out2, o2, r2, g2, k2, ks, t, rng)
        dout1 = _matmul(ds2, np.ascontiguousarray(w2.T), rng)
        dz1, ds1 = _backward(dout1, out1, o1, r1, g1, k1, ks, t, rng)
        # dW[n][k]: the chain over the rows b ascending (the reduction index of these two products is the batch row)
        dw1 = _matmul(np.ascontiguousarray(ds1.T), np.ascontiguousarray(x.T), rng)
        dw2 = _matmul(np.ascontiguousarray(ds2.T), np.ascontiguousarray(out1.T), rng)
        grads = [dw1, tile_sum(ds1, border), dw2, tile_sum(ds2, border), dw3, db3,
                 tile_sum(dz1 * o1, border), tile_sum(dz1, border), tile_sum(dz2 * o2, border), tile_sum(dz2, border)]
        new = [adam(np.asarray(p_, t), np.asarray(m_, t), np.asarray(v_, t), np.asarray(t_, t), g_, *sc)
               for p_, m_, v_, t_, g_ in zip(net, m[i], v[i], targets[i], grads)]
        out["q"].append(q)
        out["grad"].append(grads)
        for k, key in enumerate(("p", "m", "v", "target")):
            out[key].append([x_[k] for x_ in new])
        out["masks"].append((k1, k2))
    out["q"] = np.stack(out["q"])
    return out
