"""Numpy twin of the six entry points of librp_plan.so (include/plan/rp_plan.h), bit for bit: every product and every sum
is a numpy operation of its own, so each is rounded once, as in the kernels.

Philox4x32-10 is written from the algorithm of Salmon, Moraes, Dror and Shaw, "Parallel random numbers: as easy as 1, 2,
3" (SC11): ten rounds of two 32 x 32 -> 64 bit products (multipliers D2511F53, CD9E8D57), the key bumped by the Weyl
constants (9E3779B9, BB67AE85) between rounds.  The known-answer vectors below are the ones quoted in the issue that asked
for this planner, from memory of the paper's test vectors; had the algorithm disagreed with that memory, the algorithm
would have won.  It does not disagree: this implementation reproduces both (tests/test_plan_host.py).
"""

from __future__ import annotations

import numpy as np

ZERO, LINEAR = 0, 1
STEP_FIRST, STEP_MID, STEP_LAST = 0, 1, 2

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four broadcastable arrays of 32-bit words, key: two ints.  Returns four uint64 arrays of 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def z(seed_lo, seed_hi, round_, e, c):
    """The noise of rows `e` and entries `c` (broadcast against each other), float64."""
    e, c = np.asarray(e, np.uint64), np.asarray(c, np.uint64)
    S = np.zeros(np.broadcast(e, c).shape, np.uint64)
    for j in range(3):
        for w in philox4x32_10((round_, e, c, j), (seed_lo, seed_hi)):
            S = S + w
    return (S.astype(np.int64) - (np.int64(6) << np.int64(32))).astype(np.float64) * 2.0 ** -32


def knot_step(spline, p, H, P):
    if P == 1:
        return 0
    if spline == LINEAR:
        return p * ((H - 1) // (P - 1))
    return (p * H + P - 1) // P


def spline_value(knots, spline, h, H, P):
    """knots [..., P, nu] float64 -> the plan's action at control step h, [..., nu] float64."""
    knots = np.asarray(knots, np.float64)
    if P == 1:
        return knots[..., 0, :].copy()
    if spline == ZERO:
        return knots[..., min(h * P // H, P - 1), :].copy()
    assert (H - 1) % (P - 1) == 0 and H >= P
    Sd = (H - 1) // (P - 1)
    i = min(h // Sd, P - 2)
    k0, k1 = knots[..., i, :], knots[..., i + 1, :]
    w = np.float64(h - i * Sd) / np.float64(Sd)
    d = k1 - k0
    m = d * w
    return k0 + m


def fork(src, dst, K, env_first=0, env_count=None):
    """dst rows of the range <- src.repeat_interleave(K); in place, returns dst."""
    E = len(dst)
    env_count = E - env_first if env_count is None else env_count
    rows = np.arange(env_first, env_first + env_count)
    dst[rows] = src[rows // K]
    return dst


def sample(nominal, sigma, lo, hi, K, seed, round_, knots=None, env_first=0, env_count=None):
    """nominal [G, P, nu] -> knots [G K, P, nu] (rows outside the range keep what `knots` held)."""
    nominal = np.asarray(nominal, np.float64)
    G, P, nu = nominal.shape
    E = G * K
    env_count = E - env_first if env_count is None else env_count
    out = np.zeros((E, P, nu)) if knots is None else knots
    e = np.arange(E)
    c = np.arange(P * nu)
    zz = z(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, round_, e[:, None], c[None, :]).reshape(E, P, nu)
    t = np.asarray(sigma, np.float64)[None, None, :] * zz
    v = nominal[e // K] + t
    v = np.where((e % K == 0)[:, None, None], nominal[e // K], v)
    v = np.fmin(np.fmax(v, np.asarray(lo, np.float64)), np.asarray(hi, np.float64))
    rows = slice(env_first, env_first + env_count)
    out[rows] = v[rows]
    return out


def action(knots, spline, h, H, dtype=np.float64):
    knots = np.asarray(knots, np.float64)
    return spline_value(knots, spline, h, H, knots.shape[-2]).astype(dtype)


def accumulate(ret, alive, reward, step_type, weight):
    """In place on ret (float64) and alive (uint8)."""
    live = alive != 0
    t = np.float64(weight) * np.asarray(reward).astype(np.float64)
    ret[live] = (ret + t)[live]
    alive[live & (np.asarray(step_type) == STEP_LAST)] = 0
    return ret, alive


def select(ret, knots, K):
    """-> (best_k [G] int32, best_return [G], nominal [G, P, nu])."""
    ret = np.asarray(ret, np.float64).reshape(-1, K)
    G = len(ret)
    best = np.zeros(G, np.int32)
    for g in range(G):
        b = -1
        for k in range(K):
            v = ret[g, k]
            if v == v and (b < 0 or v > ret[g, b]):
                b = k
        best[g] = max(b, 0)
    rows = np.arange(G) * K + best
    return best, ret[np.arange(G), best].copy(), np.asarray(knots)[rows].copy()


def shift(nominal, spline, H):
    """nominal [G, P, nu] -> the plan one control step later (a new array)."""
    nominal = np.asarray(nominal, np.float64)
    P = nominal.shape[-2]
    out = np.empty_like(nominal)
    for p in range(P):
        out[..., p, :] = spline_value(nominal, spline, min(knot_step(spline, p, H, P) + 1, H - 1), H, P)
    return out
