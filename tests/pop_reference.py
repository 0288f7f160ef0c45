"""Numpy twins of the four entry points of librp_pop.so (include/learn/rp_pop.h): compositions of the single-learner
twins (sac_reference, droq_reference, learn_reference) over gathered inputs, with the rows and indices mapped back.  No
formula is restated here: what a member computes is what the single-learner twin computes on that member's rows.

Layouts: row j of member p of P is array row p + P j (INTERLEAVED) or p rows + j (BLOCKED).
"""

from __future__ import annotations

import numpy as np

import droq_reference as dr
import learn_reference as lr
import sac_reference as sr

INTERLEAVED, BLOCKED = 0, 1


def array_rows(p, P, rows, layout, first=0, count=None):
    """The array rows of member p's rows [first, first + count)."""
    count = rows - first if count is None else count
    j = np.arange(first, first + count)
    return p + P * j if layout == INTERLEAVED else p * rows + j


def member_ring(ring, p, P):
    """Member p's envs of the ring, gathered: every array [C, E, ...] -> [C, E / P, ...]."""
    return {k: np.ascontiguousarray(v[:, p::P]) for k, v in ring.items()}


def remap_index(index, p, P, E):
    """An index (slot Em + jj) into member p's gathered ring as the index (slot E + p + P jj) into the ring; -1 stays."""
    Em = E // P
    index = np.asarray(index, np.int64)
    return np.where(index < 0, -1, (index // Em) * E + p + P * (index % Em)).astype(np.int32)


def sample(ring, n_written, P, n, seed, round_, out=None, members=None, row_first=0, row_count=None):
    """rp_pop_sample: member p's rows are sr.sample on the gathered ring with a batch of P n, rows [p n + row_first, ...),
    the index remapped.  -> sr.sample's dict over the P n blocked rows; rows outside the ranges keep `out`."""
    E = ring["obs"].shape[1]
    assert E % P == 0
    row_count = n - row_first if row_count is None else row_count
    tries = np.zeros(P * n, np.int32)
    for p in range(P) if members is None else members:
        first = p * n + row_first
        out = sr.sample(member_ring(ring, p, P), n_written, P * n, seed, round_, out=out, row_first=first,
                        row_count=row_count)
        r = slice(first, first + row_count)
        out["index"][r] = remap_index(out["index"][r], p, P, E)
        tries[r] = out["tries"][r]   # (sr.sample starts "tries" afresh on every call)
    out["tries"] = tries
    return out


def act(obs, mean, inv_std, clip, actors, P, rows, layout, members=None, row_first=0, row_count=None, **kw):
    """rp_pop_act: member p's rows are sr.act on the whole array with member p's actor (`actors[p]`), mean[p] and
    inv_std[p], restricted to the member's array rows -- the noise is keyed by the array row.  -> {key: {array row:
    value}} flattened into arrays over all P rows rows; rows outside the ranges are NaN."""
    out = {}
    for p in range(P) if members is None else members:
        for r in array_rows(p, P, rows, layout, row_first, row_count):
            got = sr.act(obs, mean[p], inv_std[p], clip, actors[p], row_first=int(r), row_count=1, **kw)
            for k, v in got.items():
                if k not in out:
                    out[k] = np.full((P * rows,) + v.shape[1:], np.nan, v.dtype)
                out[k][r] = v[0]
    return out


def target(next_obs, action, logp, reward, discount, mean, inv_std, clip, gamma, log_alpha, critics, P, n, members=None,
           row_first=0, row_count=None, **kw):
    """rp_pop_target: member p's rows are dr.target on the batch of P n rows with row_first = p n + row_first, member
    p's critics (`critics[p]`: a sequence of ten-tuples), gamma[p], log_alpha[p], mean[p] and inv_std[p].  -> {"y",
    "q_min" [P n], "q" [n_critics, P n]}; rows outside the ranges are NaN."""
    row_count = n - row_first if row_count is None else row_count
    out = None
    for p in range(P) if members is None else members:
        first = p * n + row_first
        got = dr.target(next_obs, action, logp, reward, discount, mean[p], inv_std[p], clip, gamma[p], log_alpha[p],
                        critics[p], row_first=first, row_count=row_count, **kw)
        if out is None:
            t = got["y"].dtype
            out = {"y": np.full(P * n, np.nan, t), "q_min": np.full(P * n, np.nan, t),
                   "q": np.full((len(critics[p]), P * n), np.nan, t)}
        r = slice(first, first + row_count)
        out["y"][r], out["q_min"][r], out["q"][:, r] = got["y"], got["q_min"], got["q"]
    return out


def member_slots(obs, p, P):
    """Member p's rows of k ring slots obs [k, E, D] in the kernel's logical order r = t Em + jj: [k Em, D]."""
    k, E, D = obs.shape
    return np.ascontiguousarray(obs[:, p::P]).reshape(k * (E // P), D)


def moments(obs, count, mean, M2, eps, P):
    """rp_pop_moments: lr.moments per member on its gathered rows.  mean, M2 [P, D] -> (count, mean, M2, mean_f32,
    inv_std_f32), the last four stacked [P, D]."""
    outs = [lr.moments(member_slots(obs, p, P), count, mean[p], M2[p], eps) for p in range(P)]
    return (outs[0][0],) + tuple(np.stack([o[i] for o in outs]) for i in range(1, 5))
