"""Numpy twin of the four entry points of librp_learn.so (include/learn/rp_learn.h).

`pack` and `gae` are bit for bit: every product and every sum is a numpy operation of its own, so each is rounded once,
as in the kernels.  `act` is the same formulae in a dtype of the caller's choice: float64 is the reference, float32 the
restatement whose own error against float64 sets the bar of the kernel's.  `moments` sums with math.fsum (correctly
rounded sums), so it is a reference for the kernel's fixed-order float64 sums, not a copy.  The noise is the planner's
twin (plan_reference.z).
"""

from __future__ import annotations

import hashlib
import math

import numpy as np

import plan_reference as pr

FIRST, MID, LAST = 0, 1, 2
LN_2PI = 1.8378770664093453


# ---- pack ------------------------------------------------------------------------------------------------------------
def new_stats(E):
    return {"ep_return": np.zeros(E), "ep_len": np.zeros(E, np.int32), "done_return": np.zeros(E),
            "done_len": np.zeros(E, np.int64), "done_count": np.zeros(E, np.int32)}


def pack(fields, step_type, reward, discount, slot, stats=None, env_first=0, env_count=None):
    """fields: arrays [E, w_f] in sorted key order; slot: {"obs" [E, D] f32, "reward", "discount" [E] f32, "step_type" [E]
    i32}, written in place for the rows of the range; stats: `new_stats`, updated in place."""
    E = len(step_type)
    env_count = E - env_first if env_count is None else env_count
    rows = slice(env_first, env_first + env_count)
    slot["obs"][rows] = np.concatenate([np.asarray(f)[rows].reshape(env_count, -1).astype(np.float32) for f in fields], axis=1)
    st = np.asarray(step_type)[rows]
    r = np.zeros(env_count) if reward is None else np.asarray(reward)[rows]
    d = np.ones(env_count) if discount is None else np.asarray(discount)[rows]
    slot["step_type"][rows] = st
    slot["reward"][rows] = r.astype(np.float32)
    slot["discount"][rows] = d.astype(np.float32)
    if stats is None:
        return slot
    first, last = st == FIRST, st == LAST
    ret = np.where(first, 0.0, stats["ep_return"][rows] + r.astype(np.float64))
    length = np.where(first, 0, stats["ep_len"][rows] + 1).astype(np.int32)
    stats["ep_return"][rows], stats["ep_len"][rows] = ret, length
    stats["done_return"][rows] = np.where(last, stats["done_return"][rows] + ret, stats["done_return"][rows])
    stats["done_len"][rows] += np.where(last, length, 0)
    stats["done_count"][rows] += last.astype(np.int32)
    return slot


# ---- act -------------------------------------------------------------------------------------------------------------
def normalize(obs, mean, inv_std, clip, dtype=np.float64):
    t = dtype
    d = np.asarray(obs, t) - np.asarray(mean, t)
    p = d * np.asarray(inv_std, t)
    return np.fmin(np.fmax(p, t(-clip)), t(clip))


def mlp(x, net, dtype=np.float64):
    """net = (w1, b1, w2, b2, w3, b3), weights [out][in]."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, dtype) for a in net)
    h1 = np.tanh(np.asarray(x, dtype) @ w1.T + b1)
    h2 = np.tanh(h1 @ w2.T + b2)
    return h2 @ w3.T + b3


def noise(seed, round_, rows, A):
    """z(seed, round, e, u) for the rows `rows` and u < A, float64 [len(rows), A]."""
    return pr.z(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, round_, np.asarray(rows)[:, None], np.arange(A)[None, :])


def act(obs, mean, inv_std, clip, actor, critic, log_std=None, seed=0, round_=0, deterministic=False, dtype=np.float64,
        row_first=0, row_count=None):
    """-> dict(mu, action, logp, env_action, value) for the rows of the range (row r of the output is row row_first + r);
    `actor` / `critic` may be None."""
    t = dtype
    n = len(obs)
    row_count = n - row_first if row_count is None else row_count
    rows = np.arange(row_first, row_first + row_count)
    xn = normalize(np.asarray(obs)[rows], mean, inv_std, clip, t)
    out = {}
    if critic is not None:
        out["value"] = mlp(xn, critic, t)[:, 0]
    if actor is not None:
        mu = mlp(xn, actor, t)
        A = mu.shape[1]
        out["mu"] = mu
        if deterministic:
            a = mu
        else:
            ls = np.asarray(log_std, t)
            zf = noise(seed, round_, rows, A).astype(np.float32).astype(t)
            sd = np.exp(ls)
            a = mu + sd * zf
            g = t(-0.5) * (zf * zf) - ls
            s = np.zeros(row_count, t)
            for u in range(A):   # (ascending, as the kernel)
                s = s + g[:, u]
            out["logp"] = s - t(np.float32(0.5 * A * LN_2PI) if t is np.float32 else 0.5 * A * LN_2PI)
        out["action"] = a
        out["env_action"] = np.fmin(np.fmax(a, t(-1)), t(1))
    return out


# ---- gae -------------------------------------------------------------------------------------------------------------
def gae(reward, discount, step_type, value, gamma, lam, env_first=0, env_count=None, out=None):
    """[T+1, E] arrays -> (adv [T, E] f32, ret [T, E] f32, valid [T, E] u8); rows outside the range keep `out`."""
    reward, discount = np.asarray(reward, np.float32).astype(np.float64), np.asarray(discount, np.float32).astype(np.float64)
    V, st = np.asarray(value, np.float32).astype(np.float64), np.asarray(step_type)
    T, E = reward.shape[0] - 1, reward.shape[1]
    env_count = E - env_first if env_count is None else env_count
    adv, ret, valid = out if out is not None else (np.zeros((T, E), np.float32), np.zeros((T, E), np.float32),
                                                    np.zeros((T, E), np.uint8))
    rows = slice(env_first, env_first + env_count)
    gamma, lam = np.float64(gamma), np.float64(lam)
    carry = np.zeros(env_count)
    with np.errstate(invalid="ignore"):
        for t in range(T - 1, -1, -1):
            ok = (st[t, rows] != LAST) & (st[t + 1, rows] != FIRST)
            nv = gamma * discount[t + 1, rows]
            tv = nv * V[t + 1, rows]
            s = reward[t + 1, rows] + tv
            delta = s - V[t, rows]
            gl = nv * lam
            c = gl * carry
            A = np.where(ok, delta + c, 0.0)
            adv[t, rows] = A.astype(np.float32)
            ret[t, rows] = (A + V[t, rows]).astype(np.float32)
            valid[t, rows] = ok
            carry = A
    return adv, ret, valid


# ---- moments ---------------------------------------------------------------------------------------------------------
def batch_moments(rows):
    """(n, mean [D], M2 [D]) of the float32 rows [n, D], float64: correctly rounded sums (math.fsum); the deviations are
    taken in extended precision so that a term carries half a unit of float64 rounding at most."""
    x = np.asarray(rows, np.float32).astype(np.float64)
    n, D = x.shape
    mean = np.array([math.fsum(x[:, j]) for j in range(D)]) / n
    d = x.astype(np.longdouble) - mean.astype(np.longdouble)
    q = (d * d).astype(np.float64)
    return n, mean, np.array([math.fsum(q[:, j]) for j in range(D)])


def chan_merge(count, mean, M2, nb, mb, Mb):
    """The kernel's merge of a batch (nb, mb, Mb) into the running (count, mean, M2), operation by operation."""
    count, nb = np.float64(count), np.float64(nb)
    n = count + nb
    dl = mb - mean
    w = nb / n
    new_mean = mean + dl * w
    cross = ((dl * dl) * count) * w
    return n, new_mean, (M2 + Mb) + cross


def publish(n, mean, M2, eps):
    """(mean_f32, inv_std_f32) as the kernel publishes them."""
    var = M2 / np.float64(n)
    inv = 1.0 / np.sqrt(var + np.float64(eps))
    return mean.astype(np.float32), inv.astype(np.float32)


def moments(obs, count, mean, M2, eps):
    """One call of rp_learn_moments on the rows obs [n, D]: -> (count, mean, M2, mean_f32, inv_std_f32)."""
    nb, mb, Mb = batch_moments(obs)
    n, mean, M2 = chan_merge(count, np.asarray(mean, np.float64), np.asarray(M2, np.float64), nb, mb, Mb)
    return (n, mean, M2) + publish(n, mean, M2, eps)


# ---- a learner's checkpoint, as the layout tests of PPO and SAC compare it ------------------------------------------------
def state_tree(x):
    """The key tree of a state dict: tensors as (dtype, shape), other leaves as their type's name."""
    import torch
    if isinstance(x, torch.Tensor):
        return (str(x.dtype), tuple(x.shape))
    if isinstance(x, dict):
        return {k: state_tree(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [state_tree(v) for v in x]
    return type(x).__name__


def adam_tree(sd):
    """Of an optimizer's state dict, what is this project's: the state's keys and the parameter groups' indices."""
    return {"state": state_tree(sd["state"]), "params": [g["params"] for g in sd["param_groups"]]}


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def mlp_tree(n_in, n_out, H1=16, H2=32):
    f = "torch.float32"
    return {"0.weight": (f, (H1, n_in)), "0.bias": (f, (H1,)), "2.weight": (f, (H2, H1)), "2.bias": (f, (H2,)),
            "4.weight": (f, (n_out, H2)), "4.bias": (f, (n_out,))}
