"""Numpy twin of the three entry points of librp_sac.so (include/learn/rp_sac.h).

`sample` is bit for bit: integer arithmetic on the planner's Philox twin (plan_reference.philox4x32_10) and copies.
`act` and `target` are the header's formulae in a dtype of the caller's choice: float64 is the reference, float32 the
restatement whose own error against float64 sets the bar of the kernels'.  The normaliser, the networks and the noise
are the learner's twin (learn_reference).
"""

from __future__ import annotations

import numpy as np

import learn_reference as lr
import plan_reference as pr

FIRST, MID, LAST = lr.FIRST, lr.MID, lr.LAST
LN_2PI = lr.LN_2PI
LN_2 = 0.6931471805599453
TRIES = 4


# ---- sample ----------------------------------------------------------------------------------------------------------
def candidates(n_written, C):
    """The TimeStep numbers m that may start a transition: [n_written - F, n_written - 2], F = min(n_written, C)."""
    F = min(n_written, C)
    return np.arange(n_written - F, n_written - 1)


def valid_transitions(step_type, n_written):
    """ring step_type [C, E] -> bool [F - 1, E]: entry (t, e) is the transition that starts at TimeStep
    n_written - F + t of env e."""
    C = step_type.shape[0]
    m = candidates(n_written, C)
    return (step_type[m % C] != LAST) & (step_type[(m + 1) % C] != FIRST)


def draw(n_written, C, E, seed, round_, rows):
    """The sampler's attempts for the batch rows `rows`: (m [len(rows), TRIES], e [len(rows), TRIES])."""
    F = min(n_written, C)
    N = (F - 1) * E
    assert 0 < N < 2 ** 32
    rows = np.asarray(rows, np.uint64)
    j = np.arange(TRIES, dtype=np.uint64)
    w = pr.philox4x32_10((round_, rows[:, None], 0, np.uint64(16) + j[None, :]),
                         (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[0]
    i = (w * np.uint64(N)) >> np.uint64(32)          # (w < 2^32 and N < 2^32: the product fits 64 bits)
    t, e = (i // np.uint64(E)).astype(np.int64), (i % np.uint64(E)).astype(np.int64)
    return n_written - F + t, e


def sample(ring, n_written, B, seed, round_, out=None, row_first=0, row_count=None):
    """ring: {"obs" [C, E, D], "action" [C, E, A], "reward", "discount" [C, E], "step_type" [C, E]}.  -> {"obs",
    "next_obs" [B, D], "action" [B, A], "reward", "discount", "mask" [B] f32, "index" [B] i32, "tries" [B] (the number
    of attempts used; TRIES + 1 where none was valid; 0 outside the range)}; rows outside the range keep `out`."""
    C, E, D = ring["obs"].shape
    A = ring["action"].shape[2]
    row_count = B - row_first if row_count is None else row_count
    if out is None:
        out = {"obs": np.zeros((B, D), np.float32), "next_obs": np.zeros((B, D), np.float32),
               "action": np.zeros((B, A), np.float32), "reward": np.zeros(B, np.float32),
               "discount": np.zeros(B, np.float32), "mask": np.zeros(B, np.float32), "index": np.zeros(B, np.int32)}
    out["tries"] = np.zeros(B, np.int32)
    rows = np.arange(row_first, row_first + row_count)
    m, e = draw(n_written, C, E, seed, round_, rows)
    st = ring["step_type"]
    ok = (st[m % C, e] != LAST) & (st[(m + 1) % C, e] != FIRST)
    for b, mm, ee, good in zip(rows, m, e, ok):
        hit = np.flatnonzero(good)
        if hit.size == 0:
            for k in ("obs", "next_obs", "action", "reward", "discount", "mask"):
                out[k][b] = 0
            out["index"][b] = -1
            out["tries"][b] = TRIES + 1
            continue
        j = hit[0]
        s0, s1, en = mm[j] % C, (mm[j] + 1) % C, ee[j]
        out["obs"][b], out["next_obs"][b] = ring["obs"][s0, en], ring["obs"][s1, en]
        out["action"][b] = ring["action"][s0, en]
        out["reward"][b], out["discount"][b] = ring["reward"][s1, en], ring["discount"][s1, en]
        out["mask"][b] = 1
        out["index"][b] = s0 * E + en
        out["tries"][b] = j + 1
    return out


# ---- act -------------------------------------------------------------------------------------------------------------
def log_one_minus_tanh2(p, dtype=np.float64):
    """log(1 - tanh^2 p) as the kernel forms it: 2 (ln 2 - p - softplus(-2 p))."""
    t = dtype
    w = t(-2) * p
    sp = np.fmax(w, t(0)) + np.log1p(np.exp(-np.abs(w)))
    return t(2) * ((t(LN_2) - p) - sp)


def act(obs, mean, inv_std, clip, actor, log_std_bounds=(-5.0, 2.0), seed=0, round_=0, deterministic=False,
        dtype=np.float64, row_first=0, row_count=None):
    """-> dict(action, pre, mu, log_std, logp) for the rows of the range (row r of the output is row row_first + r)."""
    t = dtype
    n = len(obs)
    row_count = n - row_first if row_count is None else row_count
    rows = np.arange(row_first, row_first + row_count)
    xn = lr.normalize(np.asarray(obs)[rows], mean, inv_std, clip, t)
    head = lr.mlp(xn, actor, t)
    A = head.shape[1] // 2
    mu, l = head[:, :A], head[:, A:]
    ls = np.fmin(np.fmax(l, t(log_std_bounds[0])), t(log_std_bounds[1]))
    out = {"mu": mu, "log_std": ls}
    if deterministic:
        p = mu
    else:
        zf = lr.noise(seed, round_, rows, A).astype(np.float32).astype(t)
        sd = np.exp(ls)
        p = mu + sd * zf
        lg = log_one_minus_tanh2(p, t)
        g = (t(-0.5) * (zf * zf) - ls) - lg
        s = np.zeros(row_count, t)
        for u in range(A):   # (ascending, as the kernel)
            s = s + g[:, u]
        out["logp"] = s - t(np.float32(0.5 * A * LN_2PI) if t is np.float32 else 0.5 * A * LN_2PI)
    out["pre"] = p
    out["action"] = np.tanh(p)
    return out


# ---- target ----------------------------------------------------------------------------------------------------------
def q_min(next_obs, action, mean, inv_std, clip, critics, dtype=np.float64):
    t = dtype
    xa = np.concatenate([lr.normalize(next_obs, mean, inv_std, clip, t), np.asarray(action, t)], axis=1)
    qm = None
    for net in critics:   # (ascending, as the kernel)
        q = lr.mlp(xa, net, t)[:, 0]
        qm = q if qm is None else np.fmin(qm, q)
    return qm


def target(next_obs, action, logp, reward, discount, mean, inv_std, clip, gamma, log_alpha, critics, dtype=np.float64):
    """-> dict(y, q_min)."""
    t = dtype
    qm = q_min(next_obs, action, mean, inv_std, clip, critics, t)
    al = np.exp(t(np.float32(log_alpha)))
    s = al * np.asarray(logp, t)
    v = qm - s
    nv = t(np.float32(gamma)) * np.asarray(discount, t)
    tv = nv * v
    return {"y": np.asarray(reward, t) + tv, "q_min": qm}
