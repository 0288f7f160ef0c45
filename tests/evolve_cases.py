"""The case tables test_evolve_host.py and test_gpu_evolve.py share: the shapes and the data of the fold, plan and copy
cases.  Everything is drawn from numpy generators with fixed seeds, so both files see the same arrays."""

from __future__ import annotations

import numpy as np

# ---- fold ----------------------------------------------------------------------------------------------------------------
FOLD_CASES = [(1, 1), (2, 3), (3, 64), (5, 65), (8, 130), (16, 1), (256, 2)]   # (P, Em)


def fold_problem(P, Em, seed=0, big_counts=False):
    """-> dict(done_return [E] f64, done_count [E] i32, fit_sum [P] f64, fit_count [P] i64).  The returns span 1e-3 .. 1e9
    in magnitude with both signs, so another summation order gives other bits; `big_counts`: counts near 2^31 per env."""
    rng = np.random.default_rng(1000 * P + Em + 7919 * seed)
    E = P * Em
    done_return = rng.choice([-1.0, 1.0], E) * 10.0 ** rng.uniform(-3, 9, E)
    done_count = rng.integers(2 ** 31 - 1000, 2 ** 31 - 1, E, dtype=np.int64).astype(np.int32) if big_counts else \
        rng.integers(0, 5, E).astype(np.int32)
    return dict(done_return=done_return, done_count=done_count, fit_sum=rng.normal(size=P) * 1e3,
                fit_count=rng.integers(0, 100, P).astype(np.int64))


# ---- plan ----------------------------------------------------------------------------------------------------------------
PLAN_MEMBERS = [1, 2, 3, 5, 8, 16, 64, 255, 256]
PLAN_KINDS = ("spread", "tie", "mixed", "none", "inf")
PLAN_PERCENTS = (0, 1, 25, 50, 100)
MIN_EPISODES = 3


def plan_windows(P, kind, seed=0):
    """-> (fit_sum [P] f64, fit_count [P] i64) of one kind: "spread" (distinct scores), "tie" (all scores equal), "mixed"
    (a third of the members ineligible: counts below MIN_EPISODES or a NaN sum; some ties among the rest), "none" (nobody
    eligible), "inf" (+inf and -inf among the scores, two of each where P allows, so that inf - inf occurs)."""
    rng = np.random.default_rng(31 * P + 7 * PLAN_KINDS.index(kind) + 104729 * seed)
    count = rng.integers(MIN_EPISODES, 40, P).astype(np.int64)
    mean = rng.normal(size=P) * 50.0
    if kind == "tie":
        mean[:] = 2.5
        count[:] = 8          # (2.5 x 8 / 8 is exact: every score is 2.5)
    fit_sum = mean * count
    if kind == "mixed":
        which = rng.permutation(P)
        for i, p in enumerate(which[:max(P // 3, 1)]):
            if i % 3 == 0:
                count[p] = rng.integers(0, MIN_EPISODES)
            elif i % 3 == 1:
                fit_sum[p] = np.nan
            else:
                count[p] = 0
                fit_sum[p] = 0.0
        rest = which[max(P // 3, 1):]
        for a, b in zip(rest[0::4], rest[1::4]):      # pairs of equal scores: the tie rule inside a ranking
            fit_sum[b], count[b] = fit_sum[a], count[a]
    if kind == "none":
        count[:] = rng.integers(0, MIN_EPISODES, P)
        fit_sum[::2] = np.nan
    if kind == "inf":
        which = rng.permutation(P)
        for i, p in enumerate(which[:min(4, P)]):
            fit_sum[p] = np.inf if i % 2 == 0 else -np.inf
    return fit_sum, count


def plan_hypers(P, seed=0):
    """-> (gamma [P] f32, target_entropy [P] f32): a sweep."""
    rng = np.random.default_rng(17 * P + 3 + seed)
    return ((1.0 - 10.0 ** rng.uniform(-3, -1, P)).astype(np.float32), (-rng.uniform(0.5, 40.0, P)).astype(np.float32))


def plan_cases(P):
    """The argument sets of member count P: dicts of `evolve_reference.plan`'s keywords plus "windows": (kind, seed)."""
    base = dict(percent=25, min_episodes=MIN_EPISODES, min_gap=0.0, factors=(0.8, 1.25), gamma_bounds=(0.0, 0.9999),
                entropy_bounds=(-np.inf, np.inf), seed=5, generation=0, explore=("gamma", "target_entropy"))
    cases = [dict(base, windows=(kind, 0)) for kind in PLAN_KINDS]
    cases += [dict(base, windows=("spread", 1), percent=q) for q in PLAN_PERCENTS]
    cases += [dict(base, windows=("mixed", 2), percent=50), dict(base, windows=("tie", 0), percent=50)]
    cases.append(dict(base, windows=("spread", 3), percent=50, min_gap=1e9))                  # larger than every gap
    cases += [dict(base, windows=("spread", 4), percent=50, explore=e) for e in (("gamma",), ("target_entropy",), ())]
    # both clamps: every perturbed value falls below / above bounds this tight (the sweeps lie inside (0.9, 0.999) and
    # (-40, -0.5))
    cases.append(dict(base, windows=("spread", 5), percent=50, gamma_bounds=(0.9995, 0.9999), entropy_bounds=(-0.25, -0.125)))
    cases.append(dict(base, windows=("spread", 5), percent=50, gamma_bounds=(0.5, 0.75), entropy_bounds=(-100.0, -80.0)))
    cases.append(dict(base, windows=("spread", 5), percent=50, gamma_bounds=(0.95, 0.99), entropy_bounds=(-20.0, -5.0)))
    cases += [dict(base, windows=("spread", 6), percent=50, seed=s, generation=g) for s in (5, (9 << 32) + 1) for g in (0, 1, 2)]
    return cases


# ---- copy ----------------------------------------------------------------------------------------------------------------
SLICE_WORDS = [1, 2, 3, 4, 5, 7, 8, 16, 17, 1000]
BIG_SLICE = 256 * 1175
OFFSETS = (0, 4, 8, 12)            # bytes from a 16-byte boundary
FIELD_COUNTS = (1, 63, 64, 65, 130)
GUARD = 8                          # words in front of and behind every array


def copy_layout(fields, P):
    """`fields`: [(slice_words, offset_bytes)] -> (total words, [(first word, slice_words)]): the arrays [P][slice_words]
    one after the other in one buffer of 4-byte words that starts on a 16-byte boundary, each `offset_bytes` past a
    16-byte boundary with GUARD words in front of it and behind it."""
    at, out = 0, []
    for words, offset in fields:
        at += GUARD
        at = -(-at // 4) * 4 + offset // 4
        out.append((at, words))
        at += P * words
    return at + GUARD, out


def copy_buffer(total, seed=0):
    """Random words, no two slices alike."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, total, dtype=np.uint64).astype(np.uint32)


def copy_sources(P):
    """name -> source [P] int32: the identity, one loser, half the members (each takes one of the members that keep
    themselves)."""
    one = np.arange(P, dtype=np.int32)
    one[P - 1] = 0
    half = np.arange(P, dtype=np.int32)
    half[P - P // 2:] = np.arange(P // 2) % max(P - P // 2, 1)
    return {"identity": np.arange(P, dtype=np.int32), "one": one, "half": half}


def small_fields():
    """Every small slice size at every offset: 40 fields."""
    return [(w, o) for w in SLICE_WORDS for o in OFFSETS]


def counted_fields(n):
    """n fields of cycling sizes and offsets (for the chunking into launches)."""
    return [(SLICE_WORDS[i % 9], OFFSETS[(i // 3) % 4]) for i in range(n)]
