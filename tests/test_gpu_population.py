"""GPU tests of the population kernels (include/learn/rp_pop.h) and of population.DroQPopulation.

The kernel tests use one pattern.  A population kernel is the single-learner kernel's device text on a member's rows
with that member's slices of the stacked tensors; MFMA rows do not depend on their position in a tile and every other
float statement is rounded on its own.  So the population kernel must equal, BIT FOR BIT, the single-learner kernel run
per member (per row where the member's rows are interleaved) on the same array rows, and the integer twin where there is
one (tests/pop_reference.py, a composition of the single-learner twins).  Outputs start poisoned, so rows outside the
requested member and row ranges are seen untouched.  act and target are also held to the float64 twin under the bar of
test_gpu_offpolicy.py and test_gpu_droq.py: 8 times the error of a float32 numpy restatement on the same inputs,
computed by the test.

Measured on an MI355X (profiles/droq_wide_gpu_tests.txt): the target test also runs on droq_cases.WIDE_CASES (full tiles,
D + A = 16 and 64, H1 < H2, 16 <-> 256); the bits are the single-learner kernel's in every one, and the worst ratio of the
kernel's error to the restatement's per line lies between 1.2 and 2.7 there (between 1.0 and 3.6 over the four old cases).

The toy task.  `_ToyEnv` with a reward that depends on the member: -mean((a - c_p obs[:2] / 2)^2), c_p = +1 for even
members and -1 for odd ones, so one shared policy cannot be optimal for both.  The criterion is PPO's for EVERY member.
The hyper-parameters (TOY) were fixed once, before any GPU run, from a CPU restatement of the same algorithm in torch
(the class's own gradient steps on the CPU; collection, sampling and the TD target in torch) over three seeds; its
ratios and the GPU run's curve are in profiles/pop_gpu_tests.txt and at test_population_learns_a_toy_task_per_member.
"""

from __future__ import annotations

import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import droq_cases as dc  # noqa: E402
import droq_reference as dr  # noqa: E402
import pop_reference as popr  # noqa: E402
from test_gpu_offpolicy import (BOUNDS, POISON, ROUND, SEED, _differing, _dev, _host, _net, _params, _piano_env, _poisoned,  # noqa: E402
                                _ring, _run_sample, _same_bits, _snapshot, _stream, _ToyEnv, _up, _OUT)
from robopianist_amd import droq, learning, offpolicy, population  # noqa: E402
from robopianist_amd.suite.specs import TimeStep  # noqa: E402

pytestmark = pytest.mark.gpu

INTERLEAVED, BLOCKED = population.INTERLEAVED, population.BLOCKED
ORDERS = (population.TILE_MAJOR, population.MEMBER_MAJOR)


def _ids(c):
    return "x".join(map(str, c))


def _stacked(per_member):
    """A list over the members of lists of tensors -> the stacked, contiguous device tensors [P][...]."""
    return [torch.stack([t.detach() for t in ts]).contiguous().to(_dev()) for ts in zip(*per_member)]


def _bar(got, ref, f32, keys, label):
    """8 times the float32 restatement's own error against the float64 twin."""
    pairs = {k: (float(np.abs(got[k].astype(np.float64) - ref[k]).max()),
                 float(np.abs(f32[k].astype(np.float64) - ref[k]).max())) for k in keys}
    worst = max((e / b if b > 0 else (np.inf if e > 0 else 0.0)) for e, b in pairs.values())
    print(f"{label}: kernel error | float32 restatement error: " + ", ".join(f"{k} {e:.2e} | {b:.2e}" for k, (e, b) in pairs.items()) +
          f" (worst ratio: {worst:.2f})")
    for k, (e, b) in pairs.items():
        assert e <= 8 * b, (label, k, e, b)


# ---- sample ------------------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(4, 6, 5, 3, 3, 7, 3), (5, 66, 63, 45, 13, 40, 3), (3, 4, 1130, 45, 9, 33, 2), (5, 65, 63, 45, 13, 257, 1)]
_KEYS = [k for k, _, _ in _OUT]


def _run_pop_sample(ring, n_written, P, n, members=(0, None), rows=(0, None), index=True, round_=ROUND):
    C, E, D = ring["obs"].shape
    A = ring["action"].shape[2]
    d_ring = {k: _up(v) for k, v in ring.items()}
    out = {k: _up(v) for k, v in _poisoned(P * n, D, A).items()}
    population.sample(d_ring["obs"].data_ptr(), d_ring["action"].data_ptr(), d_ring["reward"].data_ptr(),
                      d_ring["discount"].data_ptr(), d_ring["step_type"].data_ptr(), out["obs"].data_ptr(),
                      out["next_obs"].data_ptr(), out["action"].data_ptr(), out["reward"].data_ptr(),
                      out["discount"].data_ptr(), out["mask"].data_ptr(), n_written, C, E, D, A, P, n,
                      index=out["index"].data_ptr() if index else None, seed=SEED, round_=round_, member_first=members[0],
                      member_count=members[1], row_first=rows[0], row_count=rows[1], hip_stream=_stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _single_learner_sample(ring, n_written, P, n):
    """rp_sac_sample per member on the gathered ring with a batch of P n and the row range [p n, p n + n), the index
    remapped; the members' launches write disjoint rows, put together here."""
    E = ring["obs"].shape[1]
    out = None
    for p in range(P):
        got = _run_sample(popr.member_ring(ring, p, P), n_written, P * n, first=p * n, count=n)
        r = slice(p * n, (p + 1) * n)
        got["index"][r] = popr.remap_index(got["index"][r], p, P, E)
        if out is None:
            out = got
        for k in _KEYS:
            out[k][r] = got[k][r]
    return out


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=_ids)
def test_sample_equals_the_single_learner_kernel_per_member_and_the_twin_bit_for_bit(case):
    C, E, D, A, n_written, n, P = case
    ring = _ring(C, E, D, A, n_written)
    got = _run_pop_sample(ring, n_written, P, n)
    want = popr.sample(ring, n_written, P, n, SEED, ROUND)
    assert [k for k in _KEYS if not _same_bits(got[k], want[k])] == []
    single = _single_learner_sample(ring, n_written, P, n)
    assert [k for k in _KEYS if not _same_bits(got[k], single[k])] == []
    drawn = got["mask"] == 1
    assert drawn.any() and ((got["index"][drawn] % E) % P == np.repeat(np.arange(P), n)[drawn]).all()
    print(f"sample {case}: {int((want['tries'] > 1).sum())} rows retried, {int((~drawn).sum())} masked")
    if P == 1:   # the single learner's kernel on the ring itself, index included
        whole = _run_sample(ring, n_written, n)
        assert [k for k in _KEYS if not _same_bits(got[k], whole[k])] == []
    # member and row sub-ranges leave the rest poisoned; no index array is accepted
    for members, rows in (((P - 1, 1), (1, n - 2)), ((0, P), (n - 1, 1)), ((0, 1), (0, n))):
        part = _run_pop_sample(ring, n_written, P, n, members=members, rows=rows, index=False)
        inside = np.zeros((P, n), bool)
        inside[members[0]:members[0] + members[1], rows[0]:rows[0] + rows[1]] = True
        inside = inside.reshape(-1)
        for k in _KEYS[:-1]:
            assert _same_bits(part[k][inside], got[k][inside]) and (part[k][~inside] == POISON).all(), (k, members, rows)
        assert (part["index"] == int(POISON)).all()
    assert not np.array_equal(_run_pop_sample(ring, n_written, P, n, round_=ROUND + 1)["index"], got["index"])


def test_sample_a_member_whose_envs_are_all_last_is_masked_and_the_others_are_not_touched():
    C, E, D, A, n_written, n, P = SAMPLE_CASES[1]
    ring = {k: v.copy() for k, v in _ring(C, E, D, A, n_written).items()}
    ring["step_type"][:, 1::P] = popr.sr.LAST
    got = _run_pop_sample(ring, n_written, P, n)
    want = popr.sample(ring, n_written, P, n, SEED, ROUND)
    assert [k for k in _KEYS if not _same_bits(got[k], want[k])] == []
    m1 = slice(n, 2 * n)
    assert (got["mask"][m1] == 0).all() and (got["index"][m1] == -1).all()
    assert all((got[k][m1] == 0).all() for k in ("obs", "next_obs", "action", "reward", "discount"))
    assert (got["mask"][:n] == 1).any() and (got["mask"][2 * n:] == 1).any()
    # members 0 and 2 draw what they draw from the ring as it was
    before = _run_pop_sample(_ring(C, E, D, A, n_written), n_written, P, n)
    for r in (slice(0, n), slice(2 * n, 3 * n)):
        assert all(_same_bits(got[k][r], before[k][r]) for k in _KEYS)


# ---- act -------------------------------------------------------------------------------------------------------------
ACT_CASES = [(1, 17, 63, 48, 16, 45), (3, 17, 63, 48, 16, 45), (2, 33, 65, 256, 256, 89), (5, 1, 1, 16, 16, 1)]
_ACT_KEYS = ("action", "pre", "env_action", "logp")


@functools.lru_cache(maxsize=None)
def _act_problem(case):
    P, rows, D, H1, H2, A = case
    rng = np.random.default_rng(sum(case))
    actors = [_net(D, H1, H2, 2 * A, 1 + rows + 7 * p) for p in range(P)]
    with torch.no_grad():   # every eleventh log-std head lies outside the bounds, above and below in turn
        for actor in actors:
            for u in range(2, A, 11):
                actor[4].bias[A + u] += 9.0 if (u // 11) % 2 == 0 else -9.0
    mean = rng.normal(size=(P, D)).astype(np.float32)
    inv_std = (1.0 / rng.uniform(0.5, 2.0, (P, D))).astype(np.float32)
    obs = (rng.normal(size=(P * rows, D)) * 2.0).astype(np.float32)
    obs.reshape(-1)[5::11] += 40.0                                    # every eleventh normalised entry clips at 5
    return types.SimpleNamespace(case=case, actors=actors, stacked=_stacked([_params(a) for a in actors]), mean=mean,
                                 inv_std=inv_std, obs=obs)


def _act_outputs(p_rows, A):
    dev = _dev()
    return {"action": torch.full((p_rows, A), POISON, device=dev), "logp": torch.full((p_rows,), POISON, device=dev),
            "pre": torch.full((p_rows, A), POISON, device=dev),
            "env_action": torch.full((p_rows, A), POISON, device=dev, dtype=torch.float64)}


def _run_pop_act(prob, layout, deterministic=False, members=(0, None), rows=(0, None), order=None):
    P, n_rows, D, H1, H2, A = prob.case
    out = _act_outputs(P * n_rows, A)
    d = {k: _up(getattr(prob, k)) for k in ("obs", "mean", "inv_std")}
    population.act(d["obs"].data_ptr(), d["mean"].data_ptr(), d["inv_std"].data_ptr(), 5.0,
                   learning.mlp_table(prob.stacked), D, H1, H2, A, P, n_rows, layout, log_std_bounds=BOUNDS,
                   action=out["action"].data_ptr(), logp=out["logp"].data_ptr(), pre=out["pre"].data_ptr(),
                   env_action=out["env_action"].data_ptr(), precision=64, deterministic=deterministic, seed=SEED,
                   round_=ROUND, member_first=members[0], member_count=members[1], row_first=rows[0], row_count=rows[1],
                   grid_order=order, hip_stream=_stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _single_learner_act(prob, layout, deterministic):
    """rp_sac_act with member p's slices: blocked, one launch per member on its row range; interleaved, one launch per
    row (row_first = r, row_count = 1) with member r % P's slices.  All into one set of poisoned outputs."""
    P, n_rows, D, H1, H2, A = prob.case
    out = _act_outputs(P * n_rows, A)
    d = {k: _up(getattr(prob, k)) for k in ("obs", "mean", "inv_std")}
    tables = [learning.mlp_table([t[p] for t in prob.stacked]) for p in range(P)]
    launches = [(p, p * n_rows, n_rows) for p in range(P)] if layout == BLOCKED else [(r % P, r, 1) for r in range(P * n_rows)]
    for p, first, count in launches:
        offpolicy.act(d["obs"].data_ptr(), d["mean"][p].data_ptr(), d["inv_std"][p].data_ptr(), 5.0, tables[p], D, H1, H2, A,
                      P * n_rows, log_std_bounds=BOUNDS, action=out["action"].data_ptr(), logp=out["logp"].data_ptr(),
                      pre=out["pre"].data_ptr(), env_action=out["env_action"].data_ptr(), precision=64,
                      deterministic=deterministic, seed=SEED, round_=ROUND, row_first=first, row_count=count,
                      hip_stream=_stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("layout", [INTERLEAVED, BLOCKED], ids=["interleaved", "blocked"])
@pytest.mark.parametrize("case", ACT_CASES, ids=_ids)
def test_act_equals_the_single_learner_kernel_per_member_bit_for_bit(case, layout):
    prob = _act_problem(case)
    P, n_rows, D, H1, H2, A = case
    for det in (False, True):
        keys = _ACT_KEYS[:3] if det else _ACT_KEYS
        got = _run_pop_act(prob, layout, det)
        single = _single_learner_act(prob, layout, det)
        assert [k for k in _ACT_KEYS if not _same_bits(got[k], single[k])] == [], (case, layout, det)
        assert all((got[k] != POISON).all() for k in keys) and (not det or (got["logp"] == POISON).all())
        assert _same_bits(got["env_action"], got["action"].astype(np.float64))
        # the grid order is a speed-only choice
        for order in ORDERS:
            other = _run_pop_act(prob, layout, det, order=order)
            assert [k for k in _ACT_KEYS if not _same_bits(got[k], other[k])] == [], (case, layout, det, order)
        # the float64 twin, under the float32 restatement's bar
        kw = dict(log_std_bounds=BOUNDS, seed=SEED, round_=ROUND, deterministic=det)
        host = [_host(a) for a in prob.actors]
        ref = popr.act(prob.obs, prob.mean, prob.inv_std, 5.0, host, P, n_rows, layout, dtype=np.float64, **kw)
        f32 = popr.act(prob.obs, prob.mean, prob.inv_std, 5.0, host, P, n_rows, layout, dtype=np.float32, **kw)
        _bar(got, ref, f32, ("action", "pre") + (() if det else ("logp",)),
             f"pop act {case} {'interleaved' if layout == INTERLEAVED else 'blocked'}{' deterministic' if det else ''}")
        # member and row sub-ranges leave the rest poisoned
        for members, rows in (((P - 1, 1), (0, n_rows)), ((0, P), (n_rows - 1, 1)), ((0, 1), (0, max(n_rows - 2, 0)))):
            part = _run_pop_act(prob, layout, det, members=members, rows=rows)
            inside = np.zeros(P * n_rows, bool)
            for p in range(members[0], members[0] + members[1]):
                inside[popr.array_rows(p, P, n_rows, layout, rows[0], rows[1])] = True
            for k in keys:
                assert _same_bits(part[k][inside], got[k][inside]) and (part[k][~inside] == POISON).all(), (k, members, rows)


# ---- target ----------------------------------------------------------------------------------------------------------
TARGET_P = (1, 3)
N_CRITICS = 3


@functools.lru_cache(maxsize=None)
def _target_problem(case, P):
    rows, D, H1, H2, A, p_drop = case
    n = rows
    rng = np.random.default_rng(1000 * P + rows + D)
    critics = [[dc.critic_net(D + A, H1, H2, p_drop, 100 * p + 10 + i + rows) for i in range(N_CRITICS)] for p in range(P)]
    mean = rng.normal(size=(P, D)).astype(np.float32)
    inv_std = (1.0 / rng.uniform(0.5, 2.0, (P, D))).astype(np.float32)
    obs = (rng.normal(size=(P * n, D)) * 2.0).astype(np.float32)
    obs.reshape(-1)[5::11] += 40.0
    kw = dict(next_obs=obs, action=np.tanh(rng.normal(size=(P * n, A))).astype(np.float32),
              logp=rng.normal(size=P * n).astype(np.float32), reward=rng.normal(size=P * n).astype(np.float32),
              discount=np.where(np.arange(P * n) % 3 == 1, 0.0, rng.uniform(0.5, 1.0, P * n)).astype(np.float32),
              mean=mean, inv_std=inv_std)
    gamma = np.float32([0.97 - 0.04 * p for p in range(P)])            # distinct values per member
    log_alpha = np.float32([-0.7 + 0.45 * p for p in range(P)])
    drop = {"on": dict(threshold=dr.drop_threshold(p_drop), keep_scale=1.0 / (1.0 - p_drop)), "off": dict(threshold=0, keep_scale=1.0)}
    return types.SimpleNamespace(case=case, P=P, n=n, critics=critics, kw=kw, gamma=gamma, log_alpha=log_alpha, drop=drop)


def _critic_stack(critics):
    """critics[p][i] -> per critic i the ten stacked tensors [P][...]."""
    return [_stacked([dc.params(member[i]) for member in critics]) for i in range(len(critics[0]))]


def _target_outputs(rows):
    dev = _dev()
    return {"y": torch.full((rows,), POISON, device=dev), "q_min": torch.full((rows,), POISON, device=dev),
            "q": torch.full((N_CRITICS, rows), POISON, device=dev)}


def _run_pop_target(prob, mode, stack=None, gamma=None, log_alpha=None, members=(0, None), rows=(0, None), order=None):
    n_rows, D, H1, H2, A, _ = prob.case
    P, n = prob.P, prob.n
    stack = _critic_stack(prob.critics) if stack is None else stack
    d = {k: _up(v) for k, v in prob.kw.items()}
    g, la = _up(prob.gamma if gamma is None else gamma), _up(prob.log_alpha if log_alpha is None else log_alpha)
    out = _target_outputs(P * n)
    population.target(d["next_obs"].data_ptr(), d["action"].data_ptr(), d["logp"].data_ptr(), d["reward"].data_ptr(),
                      d["discount"].data_ptr(), d["mean"].data_ptr(), d["inv_std"].data_ptr(), dc.CLIP, g.data_ptr(),
                      la.data_ptr(), [droq.critic_entry(ts) for ts in stack], out["y"].data_ptr(), D, H1, H2, A, P, n,
                      q_min=out["q_min"].data_ptr(), q=out["q"].data_ptr(), ln_eps=dc.LN_EPS, seed=dc.SEED, round_=dc.ROUND,
                      member_first=members[0], member_count=members[1], row_first=rows[0], row_count=rows[1],
                      grid_order=order, hip_stream=_stream(), **prob.drop[mode])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _single_learner_target(prob, mode, ranges):
    """rp_droq_target on the batch of P n rows, per member and range: row_first = p n + first, member p's critics,
    log_alpha[p] and gamma[p].  All into one set of poisoned outputs."""
    n_rows, D, H1, H2, A, _ = prob.case
    P, n = prob.P, prob.n
    stack = _critic_stack(prob.critics)
    d = {k: _up(v) for k, v in prob.kw.items()}
    la = _up(prob.log_alpha)
    out = _target_outputs(P * n)
    for p in range(P):
        entries = [droq.critic_entry([t[p] for t in ts]) for ts in stack]
        for first, count in ranges:
            droq.target(d["next_obs"].data_ptr(), d["action"].data_ptr(), d["logp"].data_ptr(), d["reward"].data_ptr(),
                        d["discount"].data_ptr(), d["mean"][p].data_ptr(), d["inv_std"][p].data_ptr(), dc.CLIP,
                        float(prob.gamma[p]), la[p:].data_ptr(), entries, out["y"].data_ptr(), D, H1, H2, A, P * n,
                        q_min=out["q_min"].data_ptr(), q=out["q"].data_ptr(), ln_eps=dc.LN_EPS, seed=dc.SEED,
                        round_=dc.ROUND, row_first=p * n + first, row_count=count, hip_stream=_stream(), **prob.drop[mode])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _flat(out):
    return dict({"y": out["y"], "q_min": out["q_min"]}, **{f"q{i}": q for i, q in enumerate(out["q"])})


@pytest.mark.parametrize("P", TARGET_P)
@pytest.mark.parametrize("case", dc.ALL_CASES, ids=dc.case_id)
def test_target_equals_the_single_learner_kernel_per_member_and_range_bit_for_bit(case, P):
    prob = _target_problem(case, P)
    n = prob.n
    B = (n + 1) // 2
    ranges = [(0, B), (B, n - B)]                                       # the utd ranges [u B, (u + 1) B)
    stop = prob.kw["discount"] == 0
    for mode in ("on", "off"):
        whole = _run_pop_target(prob, mode)
        single = _single_learner_target(prob, mode, ranges)
        assert [k for k in whole if not _same_bits(whole[k], single[k])] == [], (case, P, mode)
        assert _same_bits(whole["y"][stop], prob.kw["reward"][stop]) and stop.any()
        for first, count in ranges:   # a range by itself: the same bits, the rest poisoned
            part = _run_pop_target(prob, mode, rows=(first, count))
            inside = np.zeros((P, n), bool); inside[:, first:first + count] = True
            inside = inside.reshape(-1)
            for k in ("y", "q_min"):
                assert _same_bits(part[k][inside], whole[k][inside]) and (part[k][~inside] == POISON).all(), (k, first)
            assert _same_bits(part["q"][:, inside], whole["q"][:, inside]) and (part["q"][:, ~inside] == POISON).all()
        for order in ORDERS:
            other = _run_pop_target(prob, mode, order=order)
            assert [k for k in whole if not _same_bits(whole[k], other[k])] == [], (case, P, mode, order)
        if P > 1:
            part = _run_pop_target(prob, mode, members=(1, P - 1))
            assert (part["y"][:n] == POISON).all() and _same_bits(part["y"][n:], whole["y"][n:])
        # the float64 twin, under the float32 restatement's bar
        host = [[dc.host(c) for c in member] for member in prob.critics]
        tw = dict(clip=dc.CLIP, gamma=prob.gamma, log_alpha=prob.log_alpha, critics=host, P=P, n=n, ln_eps=dc.LN_EPS,
                  seed=dc.SEED, round_=dc.ROUND, **prob.kw, **prob.drop[mode])
        ref, f32 = _flat(popr.target(dtype=np.float64, **tw)), _flat(popr.target(dtype=np.float32, **tw))
        _bar(_flat(whole), ref, f32, list(ref), f"pop target {case} P {P} dropout {mode}")
    assert not np.array_equal(_run_pop_target(prob, "on")["q"], _run_pop_target(prob, "off")["q"])


def test_target_member_0_does_not_see_member_1s_critics_gamma_or_log_alpha():
    prob = _target_problem(dc.CASES[1], 3)
    n = prob.n
    base = _run_pop_target(prob, "on")
    stack = _critic_stack(prob.critics)
    for ts in stack:
        for t in ts:
            t[1] = t[1] * 1.5 + 0.25
    gamma, log_alpha = prob.gamma.copy(), prob.log_alpha.copy()
    gamma[1], log_alpha[1] = 0.5, 1.0
    other = _run_pop_target(prob, "on", stack=stack, gamma=gamma, log_alpha=log_alpha)
    for r in (slice(0, n), slice(2 * n, 3 * n)):
        assert _same_bits(other["y"][r], base["y"][r]) and _same_bits(other["q"][:, r], base["q"][:, r])
    live = prob.kw["discount"][n:2 * n] != 0
    assert not np.array_equal(other["y"][n:2 * n][live], base["y"][n:2 * n][live])


# ---- moments ---------------------------------------------------------------------------------------------------------
MOMENT_CASES = [(3, 5, 2, 7), (2, 70, 3, 63), (1, 65, 1, 1130)]


@pytest.mark.parametrize("case", MOMENT_CASES, ids=_ids)
def test_moments_equal_the_single_learner_kernel_on_the_gathered_rows_bit_for_bit(case):
    P, Em, k, D = case
    E = P * Em
    rng = np.random.default_rng(sum(case))
    dev = _dev()
    z = lambda dt: torch.zeros((P, D), dtype=dt, device=dev)
    pop = [z(torch.float64), z(torch.float64), z(torch.float32), torch.full((P, D), POISON, device=dev)]
    single = [[torch.zeros(D, dtype=t.dtype, device=dev) for t in pop] for _ in range(P)]
    count, tw_mean, tw_M2 = 0.0, np.zeros((P, D)), np.zeros((P, D))
    for merge in range(2):   # the second merge has count > 0
        obs = (rng.normal(size=(k, E, D)) * (1.0 + merge) + 3.0 * merge + rng.normal(size=D)).astype(np.float32)
        d_obs = _up(obs)
        population.moments(d_obs.data_ptr(), *[t.data_ptr() for t in pop], count, 1e-8, k, E, D, P, hip_stream=_stream())
        for p in range(P):
            rows = _up(popr.member_slots(obs, p, P))
            learning.moments(rows.data_ptr(), *[t.data_ptr() for t in single[p]], count, 1e-8, k * Em, D, hip_stream=_stream())
        torch.cuda.synchronize()
        count += k * Em
        for i, name in enumerate(("mean", "M2", "mean_f32", "inv_std_f32")):
            want = torch.stack([single[p][i] for p in range(P)])
            assert _same_bits(pop[i].cpu().numpy(), want.cpu().numpy()), (name, merge)
        # and the correctly rounded twin is close
        _, tw_mean, tw_M2, _, _ = popr.moments(obs, count - k * Em, tw_mean, tw_M2, 1e-8, P)
        # (a float64 chain of n terms is off by n 2^-53 times the terms' magnitudes at most; the merge adds a few roundings)
        u = (k * Em + 8) * 2.0 ** -53
        big = float(np.abs(obs).max())
        assert np.abs(pop[0].cpu().numpy() - tw_mean).max() <= 2 * u * big
        assert np.abs(pop[1].cpu().numpy() - tw_M2).max() <= 8 * u * max(float(tw_M2.max()), count * big * big)
    # a member sub-range leaves the other members' rows alone
    if P > 1:
        kept = [t.clone() for t in pop]
        population.moments(d_obs.data_ptr(), *[t.data_ptr() for t in pop], count, 1e-8, k, E, D, P, member_first=1,
                           member_count=1, hip_stream=_stream())
        torch.cuda.synchronize()
        for t, b in zip(pop, kept):
            assert torch.equal(t[0], b[0]) and torch.equal(t[2:], b[2:]) and not torch.equal(t[1], b[1])


# ---- the class on the self-actuated piano ----------------------------------------------------------------------------------
def _member_params(nets, P):
    """Per member, per network: the ten host tensors of droq_reference.target."""
    torch.cuda.synchronize()
    return [[[t.detach()[p].cpu().numpy().copy() for t in dc.params(net)] for net in nets] for p in range(P)]


def test_population_on_the_self_actuated_piano():
    E, P, C, B, utd, tau = 6, 3, 4, 16, 2, 0.25
    env_a, env_b = _piano_env(E), _piano_env(E)
    kw = dict(hidden=(32, 16), n_critics=2, capacity=C, batch_size=B, lr=1e-3, tau=tau, seed=21, utd=utd, dropout=0.5,
              gamma=[0.99, 0.9, 0.95], init_alpha=[1.0, 0.5, 0.2])
    a, b = population.DroQPopulation(env_a, P, **kw), population.DroQPopulation(env_b, P, **kw)
    # two populations from the same seed collect the same bits
    a.collect(6); b.collect(6)
    assert _differing(_snapshot(a), _snapshot(b)) == [] and a.n_written == 7
    assert a.normalizer[0] == min(7, C) * (E // P)                      # (the slots the ring still held, per member)
    assert all(torch.equal(x, y) for x, y in zip(a.normalizer[1:], b.normalizer[1:]))
    mean = a.normalizer[3].cpu().numpy()
    assert not np.array_equal(mean[0], mean[1])                         # every member has its own normaliser
    # update(1): finite statistics of length P, and every member's parameters change
    nets = [a.actor] + a.critics
    before = [t.detach().clone() for net in nets for t in net.parameters()] + [a.log_alpha.detach().clone()]
    before_range, target_range = [], a.target_range

    def hooked_target_range(u):
        before_range.append(_member_params(a.targets, P))
        return target_range(u)

    a.target_range = hooked_target_range
    round_, log_alpha = a._round, a.log_alpha.detach().cpu().numpy().copy()
    ring = _snapshot(a)
    stats = a.update(1)
    del a.target_range
    torch.cuda.synchronize()
    assert set(stats) == {"critic_loss", "actor_loss", "alpha_loss", "alpha", "entropy", "masked"}
    assert all(v.shape == (P,) and np.isfinite(v).all() for v in stats.values()), stats
    assert a._round == round_ + 1 and len(before_range) == utd
    after = [t.detach() for net in nets for t in net.parameters()] + [a.log_alpha.detach()]
    for x, y in zip(before, after):
        assert all(bool((x[p] != y[p]).any()) for p in range(P)) and bool(torch.isfinite(y).all())
    # the utd x B rows per member are the twin's, drawn in one launch from the ring as it stood
    n = utd * B
    rows = {k: v.reshape(P * n, *v.shape[2:]).cpu().numpy() for k, v in a.rows().items()}
    want = popr.sample(ring, a.n_written, P, n, a.seed, round_)
    for k in ("obs", "next_obs", "action", "reward", "discount", "mask"):
        assert _same_bits(rows[k], want[k]), k
    assert all(rows["mask"][p * n:(p + 1) * n].sum() >= 1 for p in range(P)) and all(np.isfinite(v).all() for v in rows.values())
    # y of each range: the twin on the target weights of before that range's Polyak step
    mean, inv_std = a.normalizer[3].cpu().numpy(), a.normalizer[4].cpu().numpy()
    gamma = a.gamma.cpu().numpy()
    for u in range(utd):
        tkw = dict(next_obs=rows["next_obs"], action=rows["next_action"], logp=rows["next_logp"], reward=rows["reward"],
                   discount=rows["discount"], mean=mean, inv_std=inv_std, clip=a.obs_clip, gamma=gamma, log_alpha=log_alpha,
                   critics=before_range[u], P=P, n=n, threshold=droq.drop_threshold(0.5), keep_scale=2.0, ln_eps=a.ln_eps,
                   seed=a.seed, round_=round_, row_first=u * B, row_count=B)
        ref, f32 = popr.target(dtype=np.float64, **tkw), popr.target(dtype=np.float32, **tkw)
        inside = ~np.isnan(ref["y"])
        assert inside.sum() == P * B
        got = {"y": rows["y"][inside]}
        _bar(got, {"y": ref["y"][inside]}, {"y": f32["y"][inside]}, ("y",), f"population update, range {u}")
    # actor_of(p) through the single learner's policy kernel on member p's gathered observations: that member's actions
    ts = env_b.reset()
    act = a.act(ts.observation, deterministic=True)
    torch.cuda.synchronize()
    assert tuple(act.shape) == (E, a.A) and act.dtype == torch.float64 and float(act.abs().max()) <= 1.0
    for p in range(P):
        actor = a.actor_of(p)
        obs = a._e_obs[p::P].contiguous()
        out = torch.full((E // P, a.A), POISON, device=_dev())
        env_action = torch.full((E // P, a.A), POISON, device=_dev(), dtype=torch.float64)
        _, m, _, m32, inv32 = a.normalizer_of(p)
        offpolicy.act(obs.data_ptr(), m32.data_ptr(), inv32.data_ptr(), a.obs_clip, learning.mlp_table(_params(actor)), a.D,
                      a.H1, a.H2, a.A, E // P, log_std_bounds=a.log_std_bounds, action=out.data_ptr(),
                      env_action=env_action.data_ptr(), precision=64, deterministic=True, hip_stream=_stream())
        torch.cuda.synchronize()
        assert torch.equal(env_action, act[p::P]), p
    # resume: the population's and the env's state_dict into the other pair; both continue with the same TimeSteps
    b.load_state_dict(a.state_dict())
    env_b.load_state_dict(env_a.state_dict())
    a.collect(3); b.collect(3)
    ra, rb = _snapshot(a), _snapshot(b)
    new = [m % C for m in range(a.n_written - 3, a.n_written)]
    for k in ra:
        assert _same_bits(ra[k][new], rb[k][new]), k
    assert b.n_written == a.n_written == 10 and not np.array_equal(ra["obs"], ring["obs"])
    assert all(torch.equal(x, y) for x, y in zip(a.normalizer[1:], b.normalizer[1:]))
    with pytest.raises(ValueError, match="written with members = 3"):
        population.DroQPopulation(env_b, 2, **dict(kw, gamma=0.99, init_alpha=1.0)).load_state_dict(a.state_dict())
    # the per-round statistics of train() are vectors of length P
    log = a.train(1, steps_per_round=2, grad_steps=1)
    assert all(np.shape(v) == (P,) for v in log[0].values()), {k: np.shape(v) for k, v in log[0].items()}


# ---- it learns, per member ---------------------------------------------------------------------------------------------
class _MemberToyEnv(_ToyEnv):
    """_ToyEnv (its observation and its episodes unchanged) with the reward -mean((a - c_p obs[:2] / 2)^2), c_p = +1 for
    the envs of even members and -1 for those of odd ones.  The optimum is 0 for every member; no single policy reaches
    it for both signs."""

    def __init__(self, E, seed, members):
        super().__init__(E, seed)
        member = torch.arange(E, device=_dev()) % members
        self._sign = torch.where(member % 2 == 0, 1.0, -1.0).to(torch.float32)[:, None]

    def step_canonical(self, action, bounds, clip=False):
        lo, rng = bounds
        a = lo + (action + 1.0) * 0.5 * rng
        resetting = self._needs_reset.clone()
        reward = -((a - 0.5 * self._sign * self._obs[:, :2]) ** 2).mean(1)
        self._age = torch.where(resetting, torch.zeros_like(self._age), self._age + 1)
        last = self._age >= 5
        st = torch.where(last, 2, 1).to(torch.int32)
        st = torch.where(resetting, torch.zeros_like(st), st)
        reward = torch.where(resetting, torch.zeros_like(reward), reward).contiguous()
        discount = torch.where(last & ~resetting, 0.0, 1.0).to(torch.float32).contiguous()
        self._needs_reset = last & ~resetting
        self._obs = self._draw()
        return TimeStep(st, reward, discount, {"x": self._obs})


TOY = dict(members=4, n_envs=1024, rounds=40, steps_per_round=8, grad_steps=4,
           pop=dict(hidden=(32, 32), capacity=32, batch_size=256, lr=1e-2, gamma=0.9, tau=0.05, init_alpha=0.1, seed=2, utd=4,
                    dropout=0.01))


def test_population_learns_a_toy_task_per_member():
    """PPO's criterion for every member: the mean reward of the member's last 5 of 40 rounds is at least half-way from
    that of its first 5 to the optimum 0.

    TOY was fixed before the first GPU run from the CPU restatement (seeds 2, 3, 4; four members each; last 5 / first 5):
        seed 2: 0.117 0.109 0.134 0.115     seed 3: 0.117 0.116 0.120 0.125     seed 4: 0.128 0.094 0.104 0.133
    every one below 0.25, twice the margin of the bar.  The GPU run's figures: profiles/pop_gpu_tests.txt."""
    torch.manual_seed(0)
    P = TOY["members"]
    env = _MemberToyEnv(TOY["n_envs"], seed=1, members=P)
    pop = population.DroQPopulation(env, P, **TOY["pop"])
    log = pop.train(TOY["rounds"], TOY["steps_per_round"], TOY["grad_steps"])
    curve = np.array([s["mean_reward"] for s in log])                   # [rounds, P]
    first5, last5 = curve[:5].mean(0), curve[-5:].mean(0)
    for p in range(P):
        print(f"toy task, member {p}: mean reward {first5[p]:.4f} (first 5 rounds) -> {last5[p]:.4f} (last 5); ratio "
              f"{last5[p] / first5[p]:.3f}; alpha {log[-1]['alpha'][p]:.4f}; curve {[round(float(c), 3) for c in curve[::5, p]]}")
    assert (first5 < -0.1).all() and (last5 >= 0.5 * first5).all(), (first5, last5)
    assert all(np.isfinite(s["critic_loss"]).all() for s in log) and (log[-1]["episodes"] > 0).all()
