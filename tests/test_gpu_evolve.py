"""GPU tests of population-based training (include/learn/rp_evolve.h) and of population.DroQPopulation(evolve=...).

The bar is bits everywhere: `fold`, `plan` and `copy` against the numpy twin (evolve_reference.py, written from the header
and held to hand-worked answers in test_evolve_host.py), and the learner's event against the twin and against its own
tensors before the event.  No tolerance anywhere."""

from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evolve_cases as ec  # noqa: E402
import evolve_reference as er  # noqa: E402
from test_evolve_host import _twin_kw  # noqa: E402
from test_gpu_offpolicy import _dev, _piano_env, _same_bits, _stream, _up  # noqa: E402
from robopianist_amd import evolve, population  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3   # elements behind every small array, which must keep their bits


def _guarded(x, fill):
    """`x` on the device with GUARD elements of `fill` behind it -> (the whole tensor, the view of x)."""
    x = np.ascontiguousarray(x)
    whole = _up(np.concatenate([x, np.full(GUARD, fill, x.dtype)]))
    return whole, whole[:len(x)]


def _kept(whole, fill):
    tail = whole[-GUARD:].cpu().numpy()
    return _same_bits(tail, np.full(GUARD, fill, tail.dtype))


# ---- fold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Em", ec.FOLD_CASES)
def test_fold_is_the_twin_bit_for_bit(P, Em):
    for big in (False, True):
        p = ec.fold_problem(P, Em, big_counts=big)
        E = P * Em
        ret, count = _up(p["done_return"]), _up(p["done_count"])
        w_sum, fit_sum = _guarded(p["fit_sum"], -5.5)
        w_count, fit_count = _guarded(p["fit_count"], -9)
        want = (p["fit_sum"], p["fit_count"])
        for _ in range(2):                                                               # two folds in a row accumulate
            evolve.fold(ret.data_ptr(), count.data_ptr(), fit_sum.data_ptr(), fit_count.data_ptr(), E, P, hip_stream=_stream())
            torch.cuda.synchronize()
            want = er.fold(p["done_return"], p["done_count"], want[0], want[1], P)
            assert _same_bits(fit_sum.cpu().numpy(), want[0]) and _same_bits(fit_count.cpu().numpy(), want[1]), (P, Em, big)
        assert _kept(w_sum, -5.5) and _kept(w_count, -9)
        # the env counters are left as they were
        assert _same_bits(ret.cpu().numpy(), p["done_return"]) and _same_bits(count.cpu().numpy(), p["done_count"])
        if big:
            assert (want[1] - p["fit_count"] > 2 * Em * (2 ** 31 - 1000) - 1).all() and want[1].dtype == np.int64


# ---- plan ----------------------------------------------------------------------------------------------------------------
def _run_plan(P, case):
    fit_sum, fit_count, kw = _twin_kw(case, P)
    want = er.plan(fit_sum, fit_count, **kw)
    w_sum, d_sum = _guarded(fit_sum, 4.25)
    w_count, d_count = _guarded(fit_count, 11)
    w_source, d_source = _guarded(np.full(P, -7, np.int32), -7)
    arrays = {}
    for name in ("gamma", "target_entropy"):
        arrays[name] = None if kw[name] is None else _guarded(kw[name], np.float32(0.5))
    ptr = lambda name: None if arrays[name] is None else arrays[name][1].data_ptr()
    evolve.plan(d_sum.data_ptr(), d_count.data_ptr(), d_source.data_ptr(), P, percent=kw["percent"],
                min_episodes=kw["min_episodes"], min_gap=kw["min_gap"], factors=kw["factors"], gamma=ptr("gamma"),
                gamma_bounds=kw["gamma_bounds"], target_entropy=ptr("target_entropy"), entropy_bounds=kw["entropy_bounds"],
                seed=kw["seed"], generation=kw["generation"], hip_stream=_stream())
    torch.cuda.synchronize()
    assert _same_bits(d_source.cpu().numpy(), want["source"]), (P, case, d_source.cpu().numpy(), want["source"])
    for name in ("gamma", "target_entropy"):
        if arrays[name] is not None:
            assert _same_bits(arrays[name][1].cpu().numpy(), want[name]), (P, case, name)
            assert _kept(arrays[name][0], np.float32(0.5))
    # the windows are cleared for all members, and nothing behind the arrays moved
    assert _same_bits(d_sum.cpu().numpy(), np.zeros(P)) and _same_bits(d_count.cpu().numpy(), np.zeros(P, np.int64))
    assert _kept(w_sum, 4.25) and _kept(w_count, 11) and _kept(w_source, -7)
    # a source differs from its member only for a loser, and is a winner
    source = d_source.cpu().numpy()
    for p in np.flatnonzero(source != np.arange(P)):
        assert p in want["losers"] and source[p] in want["winners"]
    return int((source != np.arange(P)).sum())


@pytest.mark.parametrize("P", ec.PLAN_MEMBERS)
def test_plan_is_the_twin_bit_for_bit(P):
    replaced = sum(_run_plan(P, case) for case in ec.plan_cases(P))
    assert replaced > 0 or P < 4


# ---- copy ----------------------------------------------------------------------------------------------------------------
def _run_copy(fields, P, source, seed=0):
    """The arrays of `ec.copy_layout(fields, P)` in one device buffer; -> the launches.  The whole buffer, guard words and
    the slices that keep themselves included, is held to the twin."""
    total, at = ec.copy_layout(fields, P)
    host = ec.copy_buffer(total, seed)
    buf = _up(host.view(np.int32))
    assert buf.data_ptr() % 16 == 0
    src = _up(np.asarray(source, np.int32))
    n = evolve.copy([(buf.data_ptr() + 4 * first, words) for first, words in at], src.data_ptr(), P, hip_stream=_stream())
    torch.cuda.synchronize()
    want = host.copy()
    changed = 0
    for first, words in at:
        view = want[first:first + P * words].reshape(P, words)
        after = er.copy(view, source)
        changed += int((after != view).any())
        view[:] = after
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), want), (len(fields), P, list(source))
    assert _same_bits(src.cpu().numpy(), np.asarray(source, np.int32))
    return n, changed


def test_copy_every_slice_size_at_every_offset():
    P = 5
    for name, source in ec.copy_sources(P).items():
        n, changed = _run_copy(ec.small_fields(), P, source, seed=1)
        assert n == 1 and (changed == 0) == (name == "identity")
    # three members, so that for odd slices a destination's alignment differs from its source's in both directions
    assert _run_copy(ec.small_fields(), 3, [0, 0, 0], seed=2) == (1, 40)
    assert _run_copy(ec.small_fields(), 3, [2, 2, 2], seed=3) == (1, 40)
    # a source that does not keep itself, or lies outside the population, copies nothing
    assert _run_copy(ec.small_fields(), 3, [1, 2, 2], seed=4)[1] == 40 and _run_copy(ec.small_fields(), 3, [1, 2, 0], seed=4)[1] == 0
    assert _run_copy(ec.small_fields(), 3, [7, -1, 2], seed=5)[1] == 0


def test_copy_the_largest_field_in_chunks():
    P = 4
    assert ec.BIG_SLICE > 73 * evolve.CHUNK_WORDS and ec.BIG_SLICE % evolve.CHUNK_WORDS
    fields = [(ec.BIG_SLICE, o) for o in ec.OFFSETS] + [(ec.BIG_SLICE + 1, 8), (ec.BIG_SLICE + 3, 4), (1, 0)]
    for name, source in ec.copy_sources(P).items():
        n, changed = _run_copy(fields, P, source, seed=6)
        assert n == 1 and changed == (0 if name == "identity" else len(fields))


@pytest.mark.parametrize("count", ec.FIELD_COUNTS)
def test_copy_chunks_its_fields_into_launches(count):
    P = 6
    for name, source in ec.copy_sources(P).items():
        n, changed = _run_copy(ec.counted_fields(count), P, source, seed=count)
        assert n == er.launches(count) == -(-count // 64) and changed == (0 if name == "identity" else count)
    assert _run_copy(ec.counted_fields(count), 1, [0])[0] == 0                           # one member: nothing to launch


def test_copy_a_stacked_float64_tensor():
    P = 4
    rng = np.random.default_rng(8)
    host = rng.normal(size=(P, 7))
    host[0, 0], host[0, 1], host[2, 2] = np.nan, -0.0, np.inf
    flat = np.concatenate([[1.5], host.ravel(), [2.5]])                                  # (a guard element either side)
    dev = _up(flat)
    src = np.array([0, 0, 2, 0], np.int32)
    d_src = _up(src)
    assert evolve.copy([(dev.data_ptr() + 8, 14)], d_src.data_ptr(), P, hip_stream=_stream()) == 1
    torch.cuda.synchronize()
    want = np.concatenate([[1.5], er.copy(host, src).ravel(), [2.5]])
    assert _same_bits(dev.cpu().numpy(), want) and not _same_bits(want, flat)


# ---- the learner on the self-actuated piano ------------------------------------------------------------------------------
P_, E_ = 4, 8
KW = dict(hidden=(16, 32), n_critics=2, capacity=4, batch_size=8, utd=2, lr=1e-3, seed=21, dropout=0.25,
          gamma=[0.99, 0.95, 0.9, 0.97], target_entropy=[-1.0, -2.0, -3.0, -4.0], init_alpha=[1.0, 0.5, 0.2, 0.1])
EVOLVE = dict(every=100, percent=50, min_episodes=2, factors=(0.8, 1.25), gamma_bounds=(0.5, 0.96), entropy_bounds=(-3.5, 0.0))
WINDOW = (np.array([10.0, 2.0, 6.0, -4.0]), np.array([2, 2, 2, 2], np.int64))     # scores 5, 1, 3, -2: 0, 2 win; 1, 3 lose


def _bits(t):
    return t.detach().cpu().numpy().copy()


def _inject(pop):
    pop._fit_sum.copy_(_up(WINDOW[0]))
    pop._fit_count.copy_(_up(WINDOW[1]))


def _twin_event(pop, gamma, entropy):
    o = pop.evolve_options
    return er.plan(WINDOW[0], WINDOW[1], percent=o["percent"], min_episodes=o["min_episodes"], min_gap=o["min_gap"],
                   factors=o["factors"], gamma=gamma if "gamma" in o["explore"] else None, gamma_bounds=o["gamma_bounds"],
                   target_entropy=entropy if "target_entropy" in o["explore"] else None, entropy_bounds=o["entropy_bounds"],
                   seed=pop.seed, generation=pop.generation)


def _policy(pop, rows):
    """`rp_pop_act`, deterministic, with the same observation rows for every member (blocked) -> [P, n, A]."""
    n = rows.shape[0]
    obs = rows.repeat(pop.P, 1).contiguous()
    out = torch.zeros(pop.P * n, pop.A, device=_dev())
    population.act(obs.data_ptr(), pop._mean_f32.data_ptr(), pop._inv_std_f32.data_ptr(), pop.obs_clip, pop._actor_table(),
                   pop.D, pop.H1, pop.H2, pop.A, pop.P, n, population.BLOCKED, log_std_bounds=pop.log_std_bounds,
                   action=out.data_ptr(), deterministic=True, seed=pop.seed, round_=pop._round, hip_stream=_stream())
    torch.cuda.synchronize()
    return out.view(pop.P, n, pop.A)


@pytest.mark.parametrize("mode", ["torch", "fused"])
def test_an_event_of_the_population_on_the_self_actuated_piano(mode):
    a = population.DroQPopulation(_piano_env(E_), P_, critic_step=mode, evolve=EVOLVE, **KW)
    torch.manual_seed(3)
    a.train(2, 2, 1)                                                                     # (every = 100: no event yet)
    assert a.generation == 0 and a._evolve_rounds == 2
    _inject(a)
    sd = a.state_dict(include_replay=True)
    torch.cuda.synchronize()
    names = [n for n, _ in a._member_fields()]
    assert len(names) == 51 + 2 * 27        # (torch: the three Adams' moments; fused: _c_m, _c_v and the two Adams left)
    assert any(n.startswith("alpha_optimizer") for n in names) and any(n.startswith("actor_optimizer") for n in names)
    before = {n: _bits(t) for n, t in a._member_fields()}
    gamma0, entropy0 = _bits(a.gamma), _bits(a.target_entropy)
    want = _twin_event(a, gamma0, entropy0)
    assert want["source"].tolist() in ([0, 0, 2, 0], [0, 0, 2, 2], [0, 2, 2, 0], [0, 2, 2, 2])
    launches = a.evolve()
    torch.cuda.synchronize()
    # the launches: the plan, and one copy launch per 64 fields
    assert launches == 1 + -(-len(names) // 64) == 3 and evolve.launches_for(len(names), P_) == 2
    source = a.last_evolution()
    assert _same_bits(source, want["source"]) and a.generation == 1
    assert _same_bits(_bits(a.gamma), want["gamma"]) and _same_bits(_bits(a.target_entropy), want["target_entropy"])
    assert not _same_bits(want["gamma"], gamma0) and not _same_bits(want["target_entropy"], entropy0)
    assert (want["gamma"][[1, 3]] <= np.float32(0.96)).all() and (want["target_entropy"][[1, 3]] >= np.float32(-3.5)).all()
    assert not bool(a._fit_sum.any()) and not bool(a._fit_count.any())
    # every field: a replaced member's slice is its source's, every other slice is what it was -- bit for bit
    after = {n: _bits(t) for n, t in a._member_fields()}
    assert list(after) == names
    for n in names:
        assert _same_bits(after[n], before[n][source]), n
    for n in ("actor.0", "critics.0.0", "targets.1.4", "log_alpha", "_mean", "_inv_std_f32"):
        assert not _same_bits(after[n][1], before[n][1]) and not _same_bits(after[n][3], before[n][3]), n
    for p in (1, 3):
        mine, theirs = a.actor_of(p).state_dict(), a.actor_of(int(source[p])).state_dict()
        assert all(torch.equal(mine[k], theirs[k]) for k in mine)
        assert all(torch.equal(x, y) for x, y in zip(a.normalizer_of(p)[1:], a.normalizer_of(int(source[p]))[1:]))
    assert not all(torch.equal(x, y) for x, y in zip(a.actor_of(0).parameters(), a.actor_of(2).parameters()))
    # the policy kernel gives a replaced member its source's actions on the same rows
    rows = torch.as_tensor(np.random.default_rng(4).normal(size=(5, a.D)).astype(np.float32), device=_dev())
    act = _policy(a, rows)
    for p in (1, 3):
        assert torch.equal(act[p], act[int(source[p])])
    assert not torch.equal(act[0], act[2])
    # training goes on
    a.collect(2)
    stats = a.update(1)
    torch.cuda.synchronize()
    assert all(np.isfinite(v).all() for v in stats.values()), stats
    assert all(bool(torch.isfinite(t).all()) for _, t in a._member_fields())
    # a state_dict taken before the event, loaded into a fresh population, reproduces the event
    b = population.DroQPopulation(_piano_env(E_), P_, critic_step=mode, evolve=EVOLVE, **dict(KW, seed=22))
    b.load_state_dict(sd)
    assert b.generation == 0 and b._evolve_rounds == 2 and b.seed == 21
    b.evolve()
    torch.cuda.synchronize()
    assert _same_bits(b.last_evolution(), source) and _same_bits(_bits(b.gamma), want["gamma"])
    assert _same_bits(_bits(b.target_entropy), want["target_entropy"])
    got = dict(b._member_fields())
    assert all(_same_bits(_bits(got[n]), after[n]) for n in names if n in got) and set(got) == set(names)


def test_each_explored_quantity_can_be_left_alone():
    env = _piano_env(E_)
    for explore in (("gamma",), ("target_entropy",), ()):
        a = population.DroQPopulation(env, P_, evolve=dict(EVOLVE, explore=explore), **KW)
        _inject(a)
        gamma0, entropy0 = _bits(a.gamma), _bits(a.target_entropy)
        want = _twin_event(a, gamma0, entropy0)
        a.evolve()
        torch.cuda.synchronize()
        assert _same_bits(a.last_evolution(), want["source"]) and (want["source"] != np.arange(P_)).sum() == 2
        assert _same_bits(_bits(a.gamma), want["gamma"] if "gamma" in explore else gamma0)
        assert _same_bits(_bits(a.target_entropy), want["target_entropy"] if "target_entropy" in explore else entropy0)
        assert ("gamma" in explore) == (not _same_bits(_bits(a.gamma), gamma0))
        assert ("target_entropy" in explore) == (not _same_bits(_bits(a.target_entropy), entropy0))


def test_train_fires_an_event_after_every_second_round():
    a = population.DroQPopulation(_piano_env(E_), P_, evolve=dict(EVOLVE, every=2), **KW)
    fired, seen, evolve_ = [], [], a.evolve
    a.evolve = lambda: (fired.append(a._evolve_rounds), evolve_())[1]
    torch.manual_seed(5)
    log = a.train(3, 2, 1, callback=lambda i, s: seen.append((i, a.generation)))
    assert fired == [2] and a.generation == 1 and len(log) == 3
    assert seen == [(0, 0), (1, 1), (2, 1)]                                              # the callback sees its round's event
    log = a.train(1, 2, 1)                                                               # the rounds are counted over the calls
    assert fired == [2, 4] and a.generation == 2 and a._evolve_rounds == 4
    assert set(log[0]) >= {"episodes", "mean_return", "mean_length", "mean_reward"} and log[0]["episodes"].shape == (P_,)
    # episode_stats folded the counters into the windows before it cleared them; the event cleared the windows
    assert not bool(a._done_count.any()) and not bool(a._fit_count.any())
    torch.cuda.synchronize()


def test_episode_stats_folds_before_it_clears():
    a = population.DroQPopulation(_piano_env(E_), P_, evolve=EVOLVE, **KW)
    off = population.DroQPopulation(_piano_env(E_), P_, **KW)
    ret = np.arange(1.0, E_ + 1.0) * 1.5
    count = np.arange(E_, dtype=np.int32) % 3
    for pop in (a, off):
        pop._done_return.copy_(_up(ret))
        pop._done_count.copy_(_up(count))
    a._fit_sum.fill_(0.25)
    stats, plain = a.episode_stats(), off.episode_stats()
    torch.cuda.synchronize()
    assert all(np.array_equal(stats[k], plain[k], equal_nan=True) for k in plain) and set(stats) == set(plain)
    want = er.fold(ret, count, np.full(P_, 0.25), np.zeros(P_, np.int64), P_)
    assert _same_bits(_bits(a._fit_sum), want[0]) and _same_bits(_bits(a._fit_count), want[1])
    assert not bool(a._done_return.any()) and not bool(a._done_count.any())
    assert stats["episodes"].tolist() == [int(count[p::P_].sum()) for p in range(P_)]
