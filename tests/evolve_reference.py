"""Numpy twin of the three entry points of librp_evolve.so, written from include/learn/rp_evolve.h statement by statement:
integers, Philox from plan_reference.py, and float64 / float32 operations one at a time, so each is rounded once, as the
header says.  Bit for bit."""

from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_reference as pr  # noqa: E402

WAVE = 64
MAX_MEMBERS, MAX_FIELDS, CHUNK_WORDS, COUNTER = 256, 64, 4096, 96


def fold(done_return, done_count, fit_sum, fit_count, P, wave=WAVE):
    """-> (fit_sum, fit_count) after the fold (new arrays).  `wave`: the lanes (64; another value shows another order)."""
    done_return, done_count = np.asarray(done_return, np.float64), np.asarray(done_count, np.int32)
    E = done_return.shape[0]
    assert E % P == 0 and done_count.shape == (E,)
    Em = E // P
    out_sum, out_count = np.array(fit_sum, np.float64), np.array(fit_count, np.int64)
    for p in range(P):
        lane_sum, lane_count = np.zeros(wave, np.float64), np.zeros(wave, np.int64)
        for l in range(wave):
            s, c = np.float64(0.0), np.int64(0)
            for j in range(l, Em, wave):
                s = s + done_return[p + P * j]
                c = c + np.int64(done_count[p + P * j])
            lane_sum[l], lane_count[l] = s, c
        t, n = np.float64(0.0), np.int64(0)
        for l in range(wave):
            t = t + lane_sum[l]
            n = n + lane_count[l]
        out_sum[p] = out_sum[p] + t
        out_count[p] = out_count[p] + n
    return out_sum, out_count


def ends(n, percent):
    """k: the size of either end among n eligible members."""
    return min(n * percent // 100, n // 2)


def scores(fit_sum, fit_count, min_episodes):
    """-> (score [P] float64, eligible [P] bool)."""
    fit_sum, fit_count = np.asarray(fit_sum, np.float64), np.asarray(fit_count, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        score = fit_sum / fit_count.astype(np.float64)
    return score, (fit_count >= min_episodes) & ~np.isnan(score)


def ranks(score, eligible):
    """-> rank [P] (-1 for an ineligible member)."""
    P = len(score)
    rank = np.full(P, -1, np.int64)
    for p in range(P):
        if eligible[p]:
            rank[p] = sum(1 for q in range(P) if eligible[q] and (score[q] > score[p] or (score[q] == score[p] and q < p)))
    return rank


def draw(seed, generation, p):
    """The four words of member p's draw."""
    return [int(w) for w in pr.philox4x32_10((generation & 0xFFFFFFFF, p, 0, COUNTER),
                                             (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))]


def explore_gamma(gamma_w, f, lo, hi):
    f32 = np.float32
    d = f32(1.0) - f32(gamma_w)
    e = d * f32(f)
    g = f32(1.0) - e
    return np.fmin(np.fmax(g, f32(lo)), f32(hi))


def explore_entropy(entropy_w, f, lo, hi):
    f32 = np.float32
    t = f32(entropy_w) * f32(f)
    return np.fmin(np.fmax(t, f32(lo)), f32(hi))


def plan(fit_sum, fit_count, percent=25, min_episodes=1, min_gap=0.0, factors=(0.8, 1.25), gamma=None,
         gamma_bounds=(0.0, 1.0), target_entropy=None, entropy_bounds=(-np.inf, np.inf), seed=0, generation=0):
    """-> dict(source int32 [P], gamma, target_entropy (new arrays or None), fit_sum, fit_count (cleared), rank, k, n,
    winners, losers)."""
    P = len(fit_sum)
    score, eligible = scores(fit_sum, fit_count, min_episodes)
    rank = ranks(score, eligible)
    n = int(eligible.sum())
    k = ends(n, percent)
    winner = {int(rank[p]): p for p in range(P) if eligible[p] and rank[p] < k}
    losers = [p for p in range(P) if eligible[p] and rank[p] >= n - k]
    source = np.arange(P, dtype=np.int32)
    new_gamma = None if gamma is None else np.array(gamma, np.float32)
    new_entropy = None if target_entropy is None else np.array(target_entropy, np.float32)
    down, up = factors
    for p in losers:
        x = draw(seed, generation, p)
        w = winner[x[0] % k]
        with np.errstate(invalid="ignore"):
            gap = score[w] - score[p]
        if not gap > np.float64(min_gap):
            continue
        source[p] = w
        if gamma is not None:
            new_gamma[p] = explore_gamma(gamma[w], up if x[1] & 1 else down, *gamma_bounds)
        if target_entropy is not None:
            new_entropy[p] = explore_entropy(target_entropy[w], up if x[1] & 2 else down, *entropy_bounds)
    return dict(source=source, gamma=new_gamma, target_entropy=new_entropy, fit_sum=np.zeros(P, np.float64),
                fit_count=np.zeros(P, np.int64), rank=rank, k=k, n=n, winners=sorted(winner.values()), losers=losers)


def copy(stacked, source):
    """`stacked`: an array [P][...] of any 4- or 8-byte dtype -> the array after the copy (a new one): slice p takes slice
    s = source[p] where 0 <= s < P, s != p and source[s] == s."""
    out = np.array(stacked)
    P = out.shape[0]
    for p in range(P):
        s = int(source[p])
        if 0 <= s < P and s != p and int(source[s]) == s:
            out[p] = stacked[s]
    return out


def launches(n_fields, P=2):
    return 0 if P == 1 else -(-n_fields // MAX_FIELDS)
