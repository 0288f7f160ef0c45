"""GPU tests of the planner (include/plan/rp_plan.h, librp_plan.so; robopianist_amd/planning.py): the six kernels against
the numpy twin (tests/plan_reference.py) bit for bit, the fork of a real environment, the invariants of
PredictiveSampler.plan(), planning in fingertip space, and PredictivePianist.

Measured on an MI355X:
  fork of a real environment (hands task, capsule fingertips, G = 2, K = 3), then 3 equal control steps of both:
      max |planning row - its real env| over qpos, reward, step type and every observation = 0 (bitwise), although the
      two engines' batch sizes differ (2 and 6); the test asserts that (4 x 0, under the hard bar of 1e-9)
  sample / action / shift / accumulate / select against the twin: bit for bit, every case
  10^5 draws of the sample kernel: mean 0.00315, variance 0.99550, max |z| 4.06
  PredictivePianist, 5 steps at G = 2, K = 8, H = 3, seeded from FingeringPianist: return 5.53 per env, running F1 0.0
      (printed, not asserted)
  recorded, not asserted (tools/gpu/plan_bench.py, profiles/plan_bench.json: G = 64, K = 64, H = 8, hull fingertips):
      one plan() 67.8 ms; 8 plain env.step calls of the same 4096-env environment 49.4 ms; the fork with its forward()
      0.30 ms; the 21 launches of librp_plan.so of one plan 0.24 ms = 0.35 % of the plan()
"""

from __future__ import annotations

import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_reference as pr  # noqa: E402
from robopianist_amd import planning  # noqa: E402

pytestmark = pytest.mark.gpu

# max |planning row - its real env| after 3 equal control steps from a fork (qpos, reward, observations); the replicas
# of a group among each other are asserted bitwise whatever this is.  0.0 = bitwise.
MEASURED_FORK_VS_REAL = 0.0
FORK_VS_REAL_BAR = 1e-9

_POISON_BYTE = 0xA5


def _dev():
    return torch.device("cuda", 0)


def _bytes(t):
    """The tensor's rows as bytes on the host, [rows, row_bytes]."""
    t = t.contiguous()
    return t.view(torch.uint8).reshape(t.shape[0], -1).cpu().numpy() if t.dtype != torch.bool else \
        t.to(torch.uint8).reshape(t.shape[0], -1).cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- fork ------------------------------------------------------------------------------------------------------------------
def _offset_by_one(make, G, row_shape):
    """A [G, *row_shape] tensor whose storage starts one element into its allocation."""
    n = int(np.prod((G,) + row_shape))
    base = make((n + 1,))
    return base[1:].view((G,) + row_shape)


@pytest.mark.parametrize("K", [1, 2, 5])
def test_fork_copies_rows_of_every_size_and_alignment(K):
    G = 3
    E = G * K
    gen = torch.Generator(device="cpu").manual_seed(K)
    f64 = lambda shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(_dev())
    i32 = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=gen, dtype=torch.int32).to(_dev())
    i64 = lambda shape: torch.randint(-2 ** 62, 2 ** 62, shape, generator=gen, dtype=torch.int64).to(_dev())
    u8 = lambda shape: torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8).to(_dev())
    boo = lambda shape: torch.randint(0, 2, shape, generator=gen, dtype=torch.uint8).bool().to(_dev())
    src = {
        "bool_1": boo((G,)), "int32_4": i32((G,)), "int64_8": i64((G,)), "f64_80": f64((G, 10)), "f64_712": f64((G, 89)),
        "f64_2136": f64((G, 267)), "u8_13": u8((G, 13)), "u8_37": u8((G, 37)),
        # one element into the allocation: 8-byte aligned rows that are never / every second time 16-aligned, odd addresses
        "f64_712_off": _offset_by_one(f64, G, (89,)), "f64_80_off": _offset_by_one(f64, G, (10,)),
        "int32_4_off": _offset_by_one(i32, G, ()), "u8_37_off": _offset_by_one(u8, G, (37,)),
        "bool_1_off": _offset_by_one(boo, G, ()),
    }
    assert src["f64_712_off"].storage_offset() == 1 and src["f64_712_off"].data_ptr() % 16 == 8
    row_bytes = {k: int(np.prod(v.shape[1:], dtype=np.int64)) * v.element_size() for k, v in src.items()}
    assert {1, 4, 8, 80, 712, 2136} <= set(row_bytes.values())
    for first, count in ((0, E), (1, max(E - 2, 1)), (E - 1, 1)):
        dst = {k: torch.full((E, row_bytes[k]), _POISON_BYTE, dtype=torch.uint8, device=_dev()) for k in src}
        # a destination one byte into its allocation as well: the byte path against aligned sources
        odd = torch.full((E * 80 + 1,), _POISON_BYTE, dtype=torch.uint8, device=_dev())
        dst["f64_80"] = odd[1:].view(E, 80)
        tab = planning.field_table([(src[k].data_ptr(), dst[k].data_ptr(), row_bytes[k]) for k in src])
        planning.fork(tab, G, K, env_first=first, env_count=count,
                      hip_stream=torch.cuda.current_stream(_dev()).cuda_stream)
        torch.cuda.synchronize()
        inside = np.zeros(E, bool); inside[first:first + count] = True
        for k in src:
            want = np.repeat(_bytes(src[k]), K, axis=0)
            got = dst[k].cpu().numpy()
            assert np.array_equal(got[inside], want[inside]), (k, K, first, count)
            assert (got[~inside] == _POISON_BYTE).all(), (k, K, first, count)


# ---- sample, action, shift -----------------------------------------------------------------------------------------
_SHAPES = [  # G, K, P, H, spline
    (2, 3, 3, 5, pr.LINEAR), (2, 3, 1, 5, pr.LINEAR), (2, 3, 2, 5, pr.ZERO), (2, 1, 3, 5, pr.LINEAR), (2, 3, 5, 5, pr.LINEAR),
    (2, 3, 3, 5, pr.ZERO), (2, 3, 1, 1, pr.ZERO)]
_NU = 45


def _problem(G, P, seed=0):
    rng = np.random.default_rng(seed)
    nominal = rng.uniform(-1, 1, (G, P, _NU))
    sigma = rng.uniform(0.05, 0.5, _NU); sigma[3] = 0.0
    lo, hi = rng.uniform(-0.9, -0.3, _NU), rng.uniform(0.3, 0.9, _NU)
    return nominal, sigma, lo, hi


def _up(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=_dev()).contiguous()


@pytest.mark.parametrize("G, K, P, H, spline", _SHAPES)
def test_sample_action_and_shift_equal_the_twin_bit_for_bit(G, K, P, H, spline):
    E = G * K
    nominal, sigma, lo, hi = _problem(G, P)
    seed, round_ = 0x1234_5678_9ABC_DEF0, 7
    d_nom, d_sig, d_lo, d_hi = _up(nominal), _up(sigma), _up(lo), _up(hi)
    st = torch.cuda.current_stream(_dev()).cuda_stream
    # -- sample, the whole batch and a sub-range into a poisoned buffer
    want = pr.sample(nominal, sigma, lo, hi, K, seed, round_)
    knots = torch.full((E, P, _NU), 7.0, dtype=torch.float64, device=_dev())
    planning.sample(d_nom.data_ptr(), d_sig.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr(), knots.data_ptr(), seed, round_,
                    G, K, P, _NU, hip_stream=st)
    got = knots.cpu().numpy()
    assert _same_bits(got, want)
    clipped = (want == lo) | (want == hi)
    assert clipped.any() and not clipped.all()                                 # bounds that actually clip
    assert _same_bits(want[::K], np.fmin(np.fmax(nominal, lo), hi))            # candidate 0: the nominal, clamped
    if K > 1:
        assert (want[1::K][..., 3] == want[::K][..., 3]).all()                  # sigma = 0: no noise
        assert not np.array_equal(want[1::K], want[2::K])
        part = torch.full((E, P, _NU), 7.0, dtype=torch.float64, device=_dev())
        planning.sample(d_nom.data_ptr(), d_sig.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr(), part.data_ptr(), seed, round_,
                        G, K, P, _NU, env_first=1, env_count=E - 2, hip_stream=st)
        part = part.cpu().numpy()
        assert _same_bits(part[1:E - 1], want[1:E - 1]) and (part[0] == 7.0).all() and (part[E - 1] == 7.0).all()
        other = torch.zeros_like(knots)
        planning.sample(d_nom.data_ptr(), d_sig.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr(), other.data_ptr(), seed,
                        round_ + 1, G, K, P, _NU, hip_stream=st)
        assert not np.array_equal(other.cpu().numpy(), want)                   # another round: other draws
    # -- action at every control step, float64 and float32 (the float64 value rounded once)
    for h in range(H):
        for prec, tdt, ndt in ((64, torch.float64, np.float64), (32, torch.float32, np.float32)):
            out = torch.full((E, _NU), 7.0, dtype=tdt, device=_dev())
            planning.action(knots.data_ptr(), out.data_ptr(), prec, spline, h, H, P, _NU, E, hip_stream=st)
            a64 = pr.action(want, spline, h, H)
            assert _same_bits(out.cpu().numpy(), a64.astype(ndt)), (h, prec)
    out = torch.full((E, _NU), 7.0, dtype=torch.float64, device=_dev())
    planning.action(knots.data_ptr(), out.data_ptr(), 64, spline, H - 1, H, P, _NU, E, row_first=E - 1, row_count=1,
                    hip_stream=st)
    out = out.cpu().numpy()
    assert (out[:E - 1] == 7.0).all() and _same_bits(out[E - 1], pr.action(want, spline, H - 1, H)[E - 1])
    # -- shift, in place, three times over; and a sub-range of groups
    cur, d_cur = nominal.copy(), _up(nominal)
    for _ in range(3):
        cur = pr.shift(cur, spline, H)
        planning.shift(d_cur.data_ptr(), spline, H, P, _NU, G, hip_stream=st)
        assert _same_bits(d_cur.cpu().numpy(), cur)
    d_one = _up(nominal)
    planning.shift(d_one.data_ptr(), spline, H, P, _NU, G, group_first=1, group_count=1, hip_stream=st)
    one = d_one.cpu().numpy()
    assert _same_bits(one[0], nominal[0]) and _same_bits(one[1], pr.shift(nominal, spline, H)[1])


def test_the_noise_of_many_rows_has_the_twins_moments():
    """10^5 draws of the kernel (sigma 1, bounds far away, nominal 0) are the twin's z, bit for bit; so they have its
    moments (tests/test_plan_host.py)."""
    G, K, P, nu = 25, 41, 2, 50          # 1025 rows of 100 entries, candidate 0 of each group left out: 100 000 draws
    zeros, ones = torch.zeros((G, P, nu), dtype=torch.float64, device=_dev()), torch.ones(nu, dtype=torch.float64, device=_dev())
    far = torch.full((nu,), 100.0, dtype=torch.float64, device=_dev())
    knots = torch.zeros((G * K, P, nu), dtype=torch.float64, device=_dev())
    planning.sample(zeros.data_ptr(), ones.data_ptr(), (-far).data_ptr(), far.data_ptr(), knots.data_ptr(), 99, 0, G, K, P, nu,
                    hip_stream=torch.cuda.current_stream(_dev()).cuda_stream)
    got = knots.cpu().numpy().reshape(G * K, P * nu)
    want = pr.z(99, 0, 0, np.arange(G * K)[:, None], np.arange(P * nu)[None, :])
    want[::K] = 0.0
    assert _same_bits(got + 0.0, want + 0.0)
    zz = got.reshape(G, K, -1)[:, 1:].ravel()
    assert zz.size == 100_000
    print(f"kernel z: mean {zz.mean():.5f} variance {zz.var():.5f} max |z| {np.abs(zz).max():.4f}")
    assert abs(zz.mean()) < 0.02 and 0.97 <= zz.var() <= 1.03 and np.abs(zz).max() <= 6.0


# ---- accumulate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_accumulate_counts_until_the_first_last_step(precision):
    tdt, ndt = (torch.float64, np.float64) if precision == 64 else (torch.float32, np.float32)
    F, M, L = pr.STEP_FIRST, pr.STEP_MID, pr.STEP_LAST
    types = np.array([[M, L, F, M],      # dies at step 1: that step counts, the new episode does not
                      [M, M, M, M],
                      [L, F, M, L],      # dies at once
                      [F, M, M, L],      # a FIRST step of its own (reward 0) does not kill
                      [M, M, L, F],
                      [M, M, M, M]], np.int32).T.copy()                       # [step, row]
    rng = np.random.default_rng(5)
    rewards = rng.uniform(0.1, 2.0, types.shape).astype(ndt)
    rewards[1, 5] = np.nan                                                   # a NaN reward: the row's return is NaN
    rewards[2, 0] = np.nan                                                   # ... but not after the row has died
    E = types.shape[1]
    ret, alive = torch.zeros(E + 2, dtype=torch.float64, device=_dev()), torch.ones(E + 2, dtype=torch.uint8, device=_dev())
    want_ret, want_alive = np.zeros(E), np.ones(E, np.uint8)
    gamma, weight = 0.9, 1.0
    st = torch.cuda.current_stream(_dev()).cuda_stream
    for h in range(types.shape[0]):
        r, t = _up(np.concatenate([rewards[h], [5, 5]]), tdt), _up(np.concatenate([types[h], [M, M]]), torch.int32)
        planning.accumulate(ret.data_ptr(), alive.data_ptr(), r.data_ptr(), t.data_ptr(), precision, weight, E + 2,
                            env_first=0, env_count=E, hip_stream=st)
        torch.cuda.synchronize()
        pr.accumulate(want_ret, want_alive, rewards[h], types[h], weight)
        weight *= gamma
    got_ret, got_alive = ret.cpu().numpy(), alive.cpu().numpy()
    assert _same_bits(got_ret[:E], want_ret) and np.array_equal(got_alive[:E], want_alive)
    assert (got_ret[E:] == 0).all() and (got_alive[E:] == 1).all()             # rows outside the range
    assert want_alive.tolist() == [0, 1, 0, 0, 0, 1]
    assert want_ret[0] == np.float64(rewards[0, 0]) + 0.9 * np.float64(rewards[1, 0])
    assert want_ret[2] == np.float64(rewards[0, 2]) and np.isnan(want_ret[5]) and np.isfinite(want_ret[:5]).all()


# ---- select ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 64, 65, 130])
def test_select_equals_the_twin(K):
    rng = np.random.default_rng(K)
    P, nu = 2, 7
    groups = []
    r = rng.normal(size=K); r[rng.integers(K)] = r.max(); r[-1] = r.max(); groups.append(r)        # a tie, the last included
    r = rng.normal(size=K); r[0] = np.nan; groups.append(r)                                        # one NaN, in front
    r = rng.normal(size=K); r[int(np.argmax(r))] = np.nan; groups.append(r)                        # one NaN, where the best was
    groups.append(np.full(K, np.nan))                                                              # all NaN
    r = np.full(K, -np.inf); r[0] = np.nan; groups.append(r)                                       # NaN, then -inf only
    r = rng.normal(size=K); r[K // 2] = -np.inf; groups.append(r)
    r = np.full(K, np.nan); r[-1] = -np.inf; groups.append(r)                                      # the only number is the last
    r = np.full(K, 1.5); groups.append(r)                                                          # all tied: the lowest
    r = rng.normal(size=K); r[-1] = r.max() + 1; groups.append(r)                                  # the best is the last
    ret = np.stack(groups).ravel()
    G = len(groups)
    knots = rng.normal(size=(G * K, P, nu))
    want_k, want_r, want_n = pr.select(ret, knots, K)
    d_ret, d_knots = _up(ret), _up(knots)
    nominal = torch.full((G + 1, P, nu), 7.0, dtype=torch.float64, device=_dev())
    best_k = torch.full((G + 1,), -5, dtype=torch.int32, device=_dev())
    best_r = torch.full((G + 1,), 7.0, dtype=torch.float64, device=_dev())
    planning.select(d_ret.data_ptr(), d_knots.data_ptr(), nominal.data_ptr(), best_k.data_ptr(), best_r.data_ptr(), G, K, P, nu,
                    hip_stream=torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()
    got_k, got_r, got_n = best_k.cpu().numpy(), best_r.cpu().numpy(), nominal.cpu().numpy()
    assert got_k[:G].tolist() == want_k.tolist(), (got_k, want_k)
    assert _same_bits(got_r[:G], want_r) and _same_bits(got_n[:G], want_n)
    assert got_k[G] == -5 and got_r[G] == 7.0 and (got_n[G] == 7.0).all()
    # what the twin is held to: NaN never wins, ties to the lowest candidate, all-NaN gives 0
    assert want_k[3] == 0 and np.isnan(want_r[3]) and want_k[7] == 0
    assert want_k[6] == K - 1 or K == 1
    assert want_k[8] == K - 1
    if K > 1:
        assert want_k[1] != 0 and want_k[4] == 1 and want_r[4] == -np.inf
        assert want_k[0] == int(np.argmax(groups[0]))                      # (numpy's argmax: the first of the tied)
    # a sub-range of groups
    best_k.fill_(-5)
    planning.select(d_ret.data_ptr(), d_knots.data_ptr(), nominal.data_ptr(), best_k.data_ptr(), best_r.data_ptr(), G, K, P, nu,
                    group_first=2, group_count=3, hip_stream=torch.cuda.current_stream(_dev()).cuda_stream)
    got_k = best_k.cpu().numpy()
    assert got_k[2:5].tolist() == want_k[2:5].tolist() and (got_k[:2] == -5).all() and (got_k[5:] == -5).all()


# ---- environments ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _load(n_envs):
    from robopianist_amd import suite
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", n_envs=n_envs, seed=3,
                          task_kwargs=dict(trim_silence=True, gravity_compensation=True, primitive_fingertip_collisions=True,
                                           n_steps_lookahead=2))


@functools.lru_cache(maxsize=None)
def _load_tips(n_envs):
    from robopianist_amd.wrappers import FingertipActionWrapper
    return FingertipActionWrapper(_load(n_envs), mode="absolute")


def _random_actions(env, n, seed):
    spec = env.action_spec()
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(spec.minimum), np.asarray(spec.maximum)
    a = lo + rng.uniform(0.3, 0.7, (n, env.n_envs, spec.shape[0])) * (hi - lo)
    return torch.as_tensor(a, device=_dev())


def _warm_up(env, steps=4, seed=11):
    """A state off the reset state, different in every env."""
    env.reset()
    for a in _random_actions(env, steps, seed):
        env.step(a)


def _flat(sd, prefix=""):
    out = {}
    for k, v in sd.items():
        if isinstance(v, dict):
            out.update(_flat(v, prefix + k + "."))
        elif isinstance(v, torch.Tensor):
            out[prefix + k] = v
    return out


def _equal_state(a, b):
    a, b = _flat(a), _flat(b)
    assert set(a) == set(b)
    return [k for k in a if not np.array_equal(_bytes(a[k]), _bytes(b[k]))]


def test_fork_of_a_real_environment_then_equal_steps():
    G, K = 2, 3
    real, plan = _load(G), _load(G * K)
    _warm_up(real)
    sampler = planning.PredictiveSampler(real, lambda n: _load(n), n_candidates=K, horizon=3, n_knots=2)
    assert sampler.plan_env is plan and len(sampler.field_names) >= 20
    plan.step(_random_actions(plan, 1, 2)[0])          # the planning env somewhere else before the fork
    sampler.fork()
    torch.cuda.synchronize()
    want, got = _flat(real.state_dict()), _flat(plan.state_dict())
    assert set(want) == set(got) and set(sampler.field_names) == set(want)
    for name in want:
        assert np.array_equal(_bytes(got[name]), np.repeat(_bytes(want[name]), K, axis=0)), name
    worst = 0.0
    for a in _random_actions(real, 3, 5):
        tr, tp = real.step(a), plan.step(a.repeat_interleave(K, dim=0))
        torch.cuda.synchronize()
        pairs = [("qpos", real.physics.qpos, plan.physics.qpos), ("reward", tr.reward, tp.reward),
                 ("step_type", tr.step_type, tp.step_type)]
        pairs += [(k, tr.observation[k], tp.observation[k]) for k in tr.observation]
        for name, r, p in pairs:
            rows = _bytes(p).reshape(G, K, -1)
            assert (rows == rows[:, :1]).all(), f"the replicas of a group differ in {name}"
            d = (p.double() - r.double().repeat_interleave(K, dim=0)).abs().max().item()
            worst = max(worst, d)
    print(f"fork then 3 equal steps: max |planning row - real env| = {worst:.3e} (recorded: {MEASURED_FORK_VS_REAL:.3e})")
    assert worst <= 4 * MEASURED_FORK_VS_REAL and worst < FORK_VS_REAL_BAR
    assert not bool(tr.first().any()) and float(tr.reward.abs().max()) > 0


def _check_plan_invariants(real, make_env, K, sigma, label):
    G, H, P = real.n_envs, 3, 2
    _warm_up(real)
    before = real.state_dict()
    s = planning.PredictiveSampler(real, make_env, n_candidates=K, horizon=H, n_knots=P, sigma=sigma, seed=17)
    first = s.plan()
    torch.cuda.synchronize()
    assert tuple(first.shape) == (G, s.nu) and first.dtype == real.physics.dtype
    assert _equal_state(before, real.state_dict()) == []                       # the real env is only read
    ret = s.returns.cpu().numpy().reshape(G, K).copy()
    best_r, best_k = s.best_return.cpu().numpy().copy(), s.best_k.cpu().numpy().copy()
    knots, nominal = s.knots.cpu().numpy().copy(), s.nominal.cpu().numpy().copy()
    print(f"{label}: returns {ret.tolist()}, best {best_k.tolist()} {best_r.tolist()}")
    assert np.isfinite(ret).all()
    for g in range(G):
        assert best_r[g] >= ret[g, 0] and best_r[g] == np.nanmax(ret[g]) and ret[g, best_k[g]] == best_r[g]
        assert _same_bits(nominal[g], knots[g * K + best_k[g]])
    assert _same_bits(first.cpu().numpy().astype(np.float64), pr.action(nominal, pr.LINEAR, 0, H))
    assert len(np.unique(ret)) > G                                             # the candidates are different plans
    # the winners again, in every row, from a fresh fork: the same return, bit for bit
    again = s.rollout(s.nominal.repeat_interleave(K, dim=0).contiguous()).cpu().numpy().reshape(G, K)
    assert _same_bits(again, np.repeat(best_r[:, None], K, axis=1)), (again, best_r)
    assert _equal_state(before, real.state_dict()) == []
    # the same seed and state: the same plan; another seed: another
    s2 = planning.PredictiveSampler(real, make_env, n_candidates=K, horizon=H, n_knots=P, sigma=sigma, seed=17)
    first2 = s2.plan().cpu().numpy()
    assert _same_bits(s2.knots.cpu().numpy(), knots) and _same_bits(s2.returns.cpu().numpy().reshape(G, K), ret)
    assert s2.best_k.cpu().numpy().tolist() == best_k.tolist() and _same_bits(first2, first.cpu().numpy())
    s3 = planning.PredictiveSampler(real, make_env, n_candidates=K, horizon=H, n_knots=P, sigma=sigma, seed=18)
    s3.plan()
    assert not np.array_equal(s3.knots.cpu().numpy(), knots)
    assert _same_bits(s3.knots.cpu().numpy()[::K], knots[::K])                  # (candidate 0 is the nominal under any seed)
    # a second round shifts the nominal and draws other noise
    s.plan()
    assert not np.array_equal(s.knots.cpu().numpy(), knots)
    assert _same_bits(s.knots.cpu().numpy()[::K], np.fmin(np.fmax(pr.shift(nominal, pr.LINEAR, H), s._lo.cpu().numpy()),
                                                            s._hi.cpu().numpy()))
    return s


def test_plan_invariants():
    _check_plan_invariants(_load(2), lambda n: _load(n), K=8, sigma=0.2, label="joint space")


def test_plan_invariants_in_fingertip_space_and_a_seeded_plan():
    from robopianist_amd.suite.fingertip_pianist import FingeringPianist
    real = _load_tips(2)
    s = _check_plan_invariants(real, lambda n: _load_tips(n), K=8, sigma=0.01, label="fingertip space")
    assert s.nu == 31
    # seeded: the nominal is FingeringPianist's action; without noise the plan returns its first action
    seed_action, weights = FingeringPianist(real, press_depth=0.01).action()
    real.set_weights(weights, validate=False)
    s.plan_env.set_weights(weights.repeat_interleave(8, dim=0), validate=False)
    quiet = planning.PredictiveSampler(real, lambda n: _load_tips(n), n_candidates=8, horizon=3, n_knots=2, sigma=0.0)
    quiet.set_nominal(seed_action)
    first = quiet.plan().cpu().numpy()
    spec = real.action_spec()
    want = np.fmin(np.fmax(seed_action.cpu().numpy(), spec.minimum), spec.maximum)
    assert _same_bits(first + 0.0, want + 0.0)
    assert float(weights.sum()) > 0 and np.abs(want).max() > 0.05
    ret = quiet.returns.cpu().numpy().reshape(2, 8)
    assert (ret == ret[:, :1]).all() and quiet.best_k.cpu().numpy().tolist() == [0, 0]   # equal plans: the lowest wins
    real.set_weights(None); s.plan_env.set_weights(None)


def test_predictive_pianist_plays_five_steps():
    """5 control steps at G = 2, K = 8, H = 3, seeded from FingeringPianist.  The return and the running F1 are printed,
    not asserted: nobody has measured what this planner achieves."""
    from robopianist_amd.suite.fingertip_pianist import FingeringPianist
    from robopianist_amd.suite.predictive_pianist import PredictivePianist
    from robopianist_amd.wrappers import MidiEvaluationWrapper
    tips = _load_tips(2)
    env = MidiEvaluationWrapper(tips)
    pianist = PredictivePianist(env, lambda n: _load_tips(n), n_candidates=8, horizon=3, n_knots=2, sigma=0.005,
                                seed_from=FingeringPianist(tips, press_depth=0.01))
    env.reset()
    total = torch.zeros(2, dtype=torch.float64, device=_dev())
    for _ in range(5):
        ts = pianist.step()
        assert bool(torch.isfinite(ts.reward).all()) and not bool(ts.last().any())
        total += ts.reward.double()
    torch.cuda.synchronize()
    f1 = (env._sums[:, 2] / torch.clamp(env._count, min=1)).cpu().numpy()
    print(f"predictive pianist, 5 steps: return {total.cpu().numpy().tolist()}, running F1 {f1.tolist()}, "
          f"best_k {pianist.sampler.best_k.cpu().numpy().tolist()}")
    assert int(env.physics.warn.max()) == 0 and int(pianist.sampler.plan_env.physics.warn.max()) == 0
    assert bool(torch.isfinite(env.physics.qpos).all())
    tips.set_weights(None); pianist.sampler.plan_env.set_weights(None)
    with pytest.raises(ValueError, match="FingertipActionWrapper"):
        PredictivePianist(_load(2), lambda n: _load(n), n_candidates=8, horizon=3, seed_from=FingeringPianist(tips, 0.01))
