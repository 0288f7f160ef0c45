"""GPU tests of the learner kernels (include/learn/rp_learn.h) and of learning.PPO.

pack and gae are compared with the numpy twin (tests/learn_reference.py) bit for bit.  moments is compared with correctly
rounded sums under a bound derived from the data.  act is compared with the float64 twin under a bar the test computes
itself: 8 times the error of a float32 numpy restatement of the same formulae on the same inputs (the kernel differs
from the twin only by float32 rounding in another order and by another tanhf / expf).

Measured on an MI355X (profiles/learn_gpu_tests.txt), kernel error | float32 restatement error against the float64 twin,
outputs of size 0.3 to 0.9:
    (rows, D, H1, H2, A)           mu                  value               action              logp
    ( 1,    1,  16,  16,   1)  1.35e-09 | 2.85e-08  2.07e-08 | 2.40e-08  1.44e-07 | 1.44e-07  3.51e-08 | 3.51e-08
    (15,    3,  16,  48,   3)  6.52e-08 | 4.58e-08  7.09e-08 | 5.90e-08  1.89e-07 | 1.69e-07  1.80e-07 | 1.80e-07
    (17,   63,  48,  16,  45)  1.43e-07 | 9.99e-08  6.33e-08 | 4.53e-08  3.72e-07 | 3.70e-07  4.01e-06 | 4.01e-06
    (33,   65, 256, 256,  89)  4.53e-07 | 4.98e-07  3.30e-07 | 1.47e-07  4.43e-07 | 4.93e-07  4.60e-06 | 4.60e-06
    (65, 1068, 256, 256,  89)  6.97e-07 | 4.79e-07  3.99e-07 | 2.11e-07  7.28e-07 | 5.57e-07  8.28e-06 | 8.28e-06
    (70, 1136,  64,  64, 128)  4.14e-07 | 4.24e-07  4.22e-07 | 2.61e-07  4.53e-07 | 4.48e-07  1.73e-05 | 1.73e-05
(the restatement's error was computed on the machine that ran the test; the bar is 8 times it).  The draws: 100,000 of
them had mean 0.00057, variance 1.00278, max |z| 4.0148.  The toy task went from a mean reward of -0.3725 over the
first 5 updates to -0.0223 over the last 5 of 40 (ratio 0.060).
"""

from __future__ import annotations

import functools
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import learn_reference as lr  # noqa: E402
from robopianist_amd import learning  # noqa: E402
from robopianist_amd.suite import specs  # noqa: E402
from robopianist_amd.suite.specs import TimeStep  # noqa: E402

pytestmark = pytest.mark.gpu

F, M, L = lr.FIRST, lr.MID, lr.LAST
POISON = -777.0


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _up(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=_dev()) if dtype is None else \
        torch.as_tensor(np.ascontiguousarray(x), device=_dev(), dtype=dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ranges(E):
    return [r for r in dict.fromkeys([(0, E), (1, E - 2), (E - 1, 1)]) if r[1] >= 0 and r[0] + r[1] <= E]


def _offset_by_one(x):
    """A device copy of x that starts one element into its allocation."""
    flat = torch.empty(x.size + 1, dtype=_up(x[:0]).dtype, device=_dev())
    flat[1:] = _up(x).reshape(-1)
    return flat[1:].view(*x.shape)


# ---- pack --------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 10, 88, 979)


def _slot(E, D, fill=POISON):
    return {"obs": np.full((E, D), fill, np.float32), "reward": np.full(E, fill, np.float32),
            "discount": np.full(E, fill, np.float32), "step_type": np.full(E, -5, np.int32)}


@pytest.mark.parametrize("E", [1, 3, 65])
def test_pack_equals_the_twin_bit_for_bit(E):
    rng = np.random.default_rng(E)
    D = sum(WIDTHS)
    for variant, (first, count) in enumerate(_ranges(E)):
        precision = (64, 32)[variant % 2]
        pdt = np.float64 if precision == 64 else np.float32
        # f32 and f64 fields; every second variant starts some sources one element into their allocation
        dtypes = [np.float32, np.float64, np.float64, np.float32] if variant % 2 == 0 else \
                 [np.float64, np.float32, np.float32, np.float64]
        fields = [(rng.normal(size=(E, w)) * 3).astype(dt) for w, dt in zip(WIDTHS, dtypes)]
        dev_fields = [_offset_by_one(f) if (variant + i) % 2 else _up(f) for i, f in enumerate(fields)]
        st = rng.integers(0, 3, E).astype(np.int32)
        reward, discount = rng.normal(size=E).astype(pdt), rng.uniform(size=E).astype(pdt)
        use_none = variant == 1 or E == 1
        want = lr.pack(fields, st, None if use_none else reward, None if use_none else discount, _slot(E, D),
                       env_first=first, env_count=count)
        got = {k: _up(v) for k, v in _slot(E, D).items()}
        d_st, d_r, d_d = _up(st), _offset_by_one(reward), _up(discount)
        tab = learning.field_table([(t.data_ptr(), w, learning.F32 if t.dtype == torch.float32 else learning.F64)
                                    for t, w in zip(dev_fields, WIDTHS)])
        learning.pack(tab, precision, d_st.data_ptr(), None if use_none else d_r.data_ptr(),
                      None if use_none else d_d.data_ptr(), got["obs"].data_ptr(), got["reward"].data_ptr(),
                      got["discount"].data_ptr(), got["step_type"].data_ptr(), E, D, env_first=first, env_count=count,
                      hip_stream=_stream())
        torch.cuda.synchronize()
        for k in want:
            assert _same_bits(got[k].cpu().numpy(), want[k]), (E, first, count, k)
        if count < E:   # (the poison outside the range is part of `want`; say so explicitly once)
            outside = np.ones(E, bool); outside[first:first + count] = False
            assert (got["obs"].cpu().numpy()[outside] == POISON).all()
        if use_none and count:
            assert (want["reward"][first:first + count] == 0).all() and (want["discount"][first:first + count] == 1).all()


def test_pack_keeps_episode_statistics():
    E = 3
    seqs = np.array([[F, M, L, F, L], [F, M, M, M, L], [M, L, F, M, M]], np.int32).T        # [step][env]
    rng = np.random.default_rng(9)
    rewards = rng.normal(size=seqs.shape)
    want, slot = lr.new_stats(E), _slot(E, 2)
    keys = ("ep_return", "ep_len", "done_return", "done_len", "done_count")
    got = {k: _up(v) for k, v in lr.new_stats(E).items()}
    dslot = {k: _up(v) for k, v in slot.items()}
    obs = np.zeros((E, 2), np.float32)
    d_obs = _up(obs)
    tab = learning.field_table([(d_obs.data_ptr(), 2, learning.F32)])
    for st, r in zip(seqs, rewards):
        lr.pack([obs], st, r, np.ones(E), slot, want)
        d_st, d_r, d_d = _up(st), _up(r), _up(np.ones(E))
        learning.pack(tab, 64, d_st.data_ptr(), d_r.data_ptr(), d_d.data_ptr(), dslot["obs"].data_ptr(),
                      dslot["reward"].data_ptr(), dslot["discount"].data_ptr(), dslot["step_type"].data_ptr(), E, 2,
                      stats=[got[k].data_ptr() for k in keys], hip_stream=_stream())
        torch.cuda.synchronize()
        for k in keys:
            assert _same_bits(got[k].cpu().numpy(), want[k]), (k, got[k], want[k])
    # env 0: FIRST MID LAST FIRST LAST = an episode of two steps and one of one step
    assert want["done_count"].tolist() == [2, 1, 1] and want["done_len"].tolist() == [3, 4, 2]
    assert want["done_return"][0] == (rewards[1, 0] + rewards[2, 0]) + rewards[4, 0]


# ---- gae ---------------------------------------------------------------------------------------------------------------
def _gae_problem(T, E, seed):
    rng = np.random.default_rng(seed)
    st = rng.choice(np.array([F, M, M, M, L], np.int32), size=(T + 1, E))
    reward = rng.normal(size=(T + 1, E)).astype(np.float32)
    value = rng.normal(size=(T + 1, E)).astype(np.float32)
    discount = np.where(rng.uniform(size=(T + 1, E)) < 0.3, 0.0, 1.0).astype(np.float32)
    if T == 9 and E >= 8:
        cols = [[L, F, M, M, M, M, M, M, M, M],      # LAST at slot 0
                [M, M, M, M, M, M, M, M, L, F],      # LAST at slot T - 1
                [M, M, M, M, M, M, M, M, M, L],      # LAST at slot T
                [M, L, F, L, F, M, M, L, F, M],      # LAST directly followed by FIRST, then LAST again
                [M, M, M, F, M, M, M, M, M, M],      # a FIRST with no LAST before it
                [M, M, L, F, M, M, L, F, M, M],      # discount 0 at the first LAST, 1 at the second
                [M, M, L, F, M, M, L, F, M, M]]      # the NaN column (below)
        for e, c in enumerate(cols):
            st[:, e] = c
        discount[2, 5], discount[6, 5] = 0.0, 1.0
        discount[:, 6] = 1.0
    return reward, discount, st, value


def _run_gae(reward, discount, st, value, gamma, lam, first, count):
    T, E = reward.shape[0] - 1, reward.shape[1]
    adv, ret = _up(np.full((T, E), POISON, np.float32)), _up(np.full((T, E), POISON, np.float32))
    valid = _up(np.full((T, E), 9, np.uint8))
    d = [_up(x) for x in (reward, discount, st, value)]
    learning.gae(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), adv.data_ptr(), ret.data_ptr(),
                 valid.data_ptr(), gamma, lam, T, E, env_first=first, env_count=count, hip_stream=_stream())
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy(), valid.cpu().numpy()


def _equal_or_both_nan(a, b):
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and _same_bits(np.where(nan, 0, a), np.where(nan, 0, b))


@pytest.mark.parametrize("T", [1, 2, 9])
@pytest.mark.parametrize("E", [1, 65])
def test_gae_equals_the_twin_bit_for_bit(T, E):
    reward, discount, st, value = _gae_problem(T, E, 100 * T + E)
    for first, count in _ranges(E):
        out = (np.full((T, E), POISON, np.float32), np.full((T, E), POISON, np.float32), np.full((T, E), 9, np.uint8))
        want = lr.gae(reward, discount, st, value, 0.99, 0.95, first, count, out=out)
        got = _run_gae(reward, discount, st, value, 0.99, 0.95, first, count)
        for g, w in zip(got, want):
            assert _same_bits(g, w), (T, E, first, count)
    if T == 9 and E == 65:
        adv, ret, valid = _run_gae(reward, discount, st, value, 0.99, 0.95, 0, E)
        assert valid[:, 0].tolist() == [0] + [1] * 8 and valid[:, 1].tolist() == [1] * 8 + [0]
        assert valid[:, 2].tolist() == [1] * 9 and valid[:, 3].tolist() == [1, 0, 1, 0, 1, 1, 1, 0, 1]
        assert valid[:, 4].tolist() == [1, 1, 0, 1, 1, 1, 1, 1, 1]
        # a NaN reward inside the second episode (slots 3 .. 6) of env 6: that episode's slots before it turn NaN, the
        # other episodes of the env and every other env keep their bits
        bad = reward.copy()
        bad[5, 6] = np.nan
        adv2, ret2, valid2 = _run_gae(bad, discount, st, value, 0.99, 0.95, 0, E)
        w2 = lr.gae(bad, discount, st, value, 0.99, 0.95)
        assert _equal_or_both_nan(adv2, w2[0]) and _equal_or_both_nan(ret2, w2[1]) and _same_bits(valid2, valid)
        assert np.isnan(adv2[3:5, 6]).all() and np.isnan(adv2).sum() == 2
        keep = ~np.isnan(adv2)
        assert np.array_equal(adv2[keep].view(np.uint32), adv[keep].view(np.uint32))
        assert np.array_equal(ret2[keep].view(np.uint32), ret[keep].view(np.uint32))


# ---- moments -----------------------------------------------------------------------------------------------------------
U = 2.0 ** -53


def _moments_call(obs, count, mean, M2, eps=1e-8):
    n, D = obs.shape
    d_obs = _up(obs)
    mean32, inv32 = _up(np.full(D, POISON, np.float32)), _up(np.full(D, POISON, np.float32))
    learning.moments(d_obs.data_ptr(), mean.data_ptr(), M2.data_ptr(), mean32.data_ptr(), inv32.data_ptr(), count, eps, n, D,
                     hip_stream=_stream())
    torch.cuda.synchronize()
    return mean32.cpu().numpy(), inv32.cpu().numpy()


@pytest.mark.parametrize("n, D", [(1, 1), (7, 3), (130, 65), (16 * 70, 1068)])
def test_moments_stay_inside_the_summation_bound_and_repeat_bit_for_bit(n, D):
    """Any order of summing m float64 terms errs by at most m 2^-53 sum|term|.  After each of two merges the kernel's
    running mean and M2 are compared with correctly rounded sums over all m rows merged so far:
    |mean - ref| <= m u sum|x| / m and |M2 - ref| <= m u sum (x - mean)^2, u = 2^-53, both computed from the data."""
    rng = np.random.default_rng(n + D)
    scale, shift = rng.uniform(0.1, 5, D), rng.normal(size=D) * 3
    batches = [(rng.normal(size=(n, D)) * scale + shift).astype(np.float32) for _ in range(2)]
    runs = []
    for _ in range(2):
        mean, M2 = _up(np.zeros(D)), _up(np.zeros(D))
        count, trace = 0.0, []
        for b in batches:
            mean32, inv32 = _moments_call(b, count, mean, M2)
            count += n
            trace.append((mean.cpu().numpy().copy(), M2.cpu().numpy().copy(), mean32, inv32))
        runs.append(trace)
    worst = [0.0, 0.0]
    for k in range(2):
        rows = np.concatenate(batches[:k + 1])
        m, ref_mean, ref_M2 = lr.batch_moments(rows)
        x = rows.astype(np.float64)
        bound_mean = m * U * np.abs(x).sum(0) / m
        bound_M2 = m * U * ((x - ref_mean) ** 2).sum(0)
        mean, M2, mean32, inv32 = runs[0][k]
        err_mean, err_M2 = np.abs(mean - ref_mean), np.abs(M2 - ref_M2)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[0] = max(worst[0], np.nanmax(np.where(bound_mean > 0, err_mean / bound_mean, 0)))
            worst[1] = max(worst[1], np.nanmax(np.where(bound_M2 > 0, err_M2 / bound_M2, 0)))
        assert (err_mean <= bound_mean).all(), (n, D, k, (err_mean / bound_mean).max())
        assert (err_M2 <= bound_M2).all(), (n, D, k)
        want32 = lr.publish(m, mean, M2, 1e-8)
        assert _same_bits(mean32, want32[0]) and _same_bits(inv32, want32[1])
        for a, b in zip(runs[0][k], runs[1][k]):
            assert _same_bits(a, b)
    print(f"moments ({n}, {D}): worst error / bound: mean {worst[0]:.3f}, M2 {worst[1]:.3f}")


# ---- act ---------------------------------------------------------------------------------------------------------------
ACT_CASES = [(1, 1, 16, 16, 1), (15, 3, 16, 48, 3), (17, 63, 48, 16, 45), (33, 65, 256, 256, 89),
             (65, 1068, 256, 256, 89), (70, 1136, 64, 64, 128)]


def _net(D, H1, H2, A, seed):
    """Weights drawn as nn.Linear draws them."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(D, H1), torch.nn.Tanh(), torch.nn.Linear(H1, H2), torch.nn.Tanh(),
                                   torch.nn.Linear(H2, A))


def _params(net):
    return [t for i in (0, 2, 4) for t in (net[i].weight, net[i].bias)]


@functools.lru_cache(maxsize=None)
def _act_problem(case):
    """The inputs of a case, its float64 twin, and the float32 restatement's error against it -- computed once."""
    rows, D, H1, H2, A = case
    rng = np.random.default_rng(sum(case))
    actor, critic = _net(D, H1, H2, A, 1 + rows), _net(D, H1, H2, 1, 2 + rows)
    mean = rng.normal(size=D).astype(np.float32)
    inv_std = (1.0 / rng.uniform(0.5, 2.0, D)).astype(np.float32)
    obs = (mean + rng.normal(size=(rows, D)) * 2.0).astype(np.float32)
    obs.reshape(-1)[5::11] += 40.0                                    # every eleventh normalised entry clips at 5
    log_std = rng.uniform(-1.0, 0.3, A).astype(np.float32)
    wa, wc = [p.detach().numpy() for p in _params(actor)], [p.detach().numpy() for p in _params(critic)]
    kw = dict(obs=obs, mean=mean, inv_std=inv_std, clip=5.0, actor=wa, critic=wc, log_std=log_std, seed=(7 << 32) | 11,
              round_=3)
    ref = lr.act(dtype=np.float64, **kw)
    f32 = lr.act(dtype=np.float32, **kw)
    err32 = {k: float(np.abs(f32[k].astype(np.float64) - ref[k]).max()) for k in ("mu", "value", "action", "logp")}
    clipped = float((np.abs(lr.normalize(obs, mean, inv_std, 5.0)) == 5.0).mean())
    return types.SimpleNamespace(case=case, actor=actor, critic=critic, mean=mean, inv_std=inv_std, obs=obs,
                                 log_std=log_std, ref=ref, err32=err32, kw=kw, clipped=clipped)


def _run_act(p, precision=64, deterministic=False, first=0, count=None, seed=None, round_=None, actor=True, critic=True,
             nets=None):
    rows, D, H1, H2, A = p.case
    dev = _dev()
    a_net, c_net = nets if nets is not None else (p.actor.to(dev), p.critic.to(dev))
    edt = torch.float32 if precision == 32 else torch.float64
    out = {"action": torch.full((rows, A), POISON, device=dev), "logp": torch.full((rows,), POISON, device=dev),
           "mu": torch.full((rows, A), POISON, device=dev), "value": torch.full((rows,), POISON, device=dev),
           "env_action": torch.full((rows, A), POISON, device=dev, dtype=edt)}
    d = {k: _up(getattr(p, k)) for k in ("obs", "mean", "inv_std", "log_std")}
    learning.act(d["obs"].data_ptr(), d["mean"].data_ptr(), d["inv_std"].data_ptr(), 5.0,
                 learning.mlp_table(_params(a_net)) if actor else None, learning.mlp_table(_params(c_net)) if critic else None,
                 D, H1, H2, A, rows, log_std=d["log_std"].data_ptr(), action=out["action"].data_ptr(),
                 logp=out["logp"].data_ptr(), mu=out["mu"].data_ptr(), env_action=out["env_action"].data_ptr(),
                 value=out["value"].data_ptr(), precision=precision, deterministic=deterministic,
                 seed=p.kw["seed"] if seed is None else seed, round_=p.kw["round_"] if round_ is None else round_,
                 row_first=first, row_count=count, hip_stream=_stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", ACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_act_equals_the_float64_twin_within_8_float32_restatement_errors(case):
    p = _act_problem(case)
    rows, D, H1, H2, A = case
    assert D < 3 or p.clipped > 0.01
    got = _run_act(p)
    report = []
    for k in ("mu", "value", "action", "logp"):
        err = float(np.abs(got[k].astype(np.float64) - p.ref[k]).max())
        report.append(f"{k} {err:.2e} | {p.err32[k]:.2e}")
    print(f"act {case}: kernel error | float32 restatement error: " + ", ".join(report)
          + f"; |outputs| up to {max(np.abs(p.ref['mu']).max(), np.abs(p.ref['value']).max()):.2f}")
    for k in ("mu", "value", "action", "logp"):
        err = float(np.abs(got[k].astype(np.float64) - p.ref[k]).max())
        assert err <= 8 * p.err32[k], (k, err, p.err32[k])
    # the env's action is the clamp of the stored action, exactly, in both precisions
    assert _same_bits(got["env_action"], np.fmin(np.fmax(got["action"], -1), 1).astype(np.float64))
    got32 = _run_act(p, precision=32)
    assert _same_bits(got32["env_action"], np.fmin(np.fmax(got32["action"], np.float32(-1)), np.float32(1)))
    assert (np.abs(got["action"]) > 1).any() or A < 3
    # the same arguments give the same bits twice
    for k in ("action", "logp", "mu", "value"):
        assert _same_bits(got[k], got32[k]), k
    # torch's own forward of the same modules on the GPU
    with torch.no_grad():
        xn = torch.clamp((_up(p.obs) - _up(p.mean)) * _up(p.inv_std), -5.0, 5.0)
        t_mu, t_v = p.actor.to(_dev())(xn).cpu().numpy(), p.critic.to(_dev())(xn)[:, 0].cpu().numpy()
    e_mu, e_v = np.abs(got["mu"].astype(np.float64) - t_mu).max(), np.abs(got["value"].astype(np.float64) - t_v).max()
    print(f"act {case}: against torch's forward on the GPU: mu {e_mu:.2e}, value {e_v:.2e}")
    assert e_mu <= 8 * p.err32["mu"] and e_v <= 8 * p.err32["value"]


@pytest.mark.parametrize("case", [ACT_CASES[2], ACT_CASES[4]], ids=lambda c: "x".join(map(str, c)))
def test_act_row_ranges_modes_and_draws(case):
    p = _act_problem(case)
    rows, D, H1, H2, A = case
    full = _run_act(p)
    for first, count in _ranges(rows):
        got = _run_act(p, first=first, count=count)
        inside = np.zeros(rows, bool); inside[first:first + count] = True
        for k in ("action", "logp", "mu", "value", "env_action"):
            assert _same_bits(got[k][inside], full[k][inside]), (k, first, count)
            assert (got[k][~inside] == POISON).all(), (k, first, count)
    det = _run_act(p, deterministic=True)
    assert _same_bits(det["action"], full["mu"]) and _same_bits(det["mu"], full["mu"]) and (det["logp"] == POISON).all()
    assert _same_bits(det["value"], full["value"])
    only_v = _run_act(p, actor=False)
    assert _same_bits(only_v["value"], full["value"]) and (only_v["action"] == POISON).all() and (only_v["mu"] == POISON).all()
    only_a = _run_act(p, critic=False)
    assert _same_bits(only_a["action"], full["action"]) and (only_a["value"] == POISON).all()
    for other in (dict(round_=4), dict(seed=(7 << 32) | 12), dict(seed=(8 << 32) | 11)):
        o = _run_act(p, **other)
        assert _same_bits(o["mu"], full["mu"]) and not np.array_equal(o["action"], full["action"])
        assert not np.array_equal(o["logp"], full["logp"])


def test_act_draws_the_planners_noise_1e5_draws():
    """A zero head and log_std = 0 make the action the draw itself: (float)z of the planner's twin, bit for bit."""
    rows, D, H1, H2, A = 1000, 5, 16, 16, 100
    p = _act_problem((rows, D, H1, H2, A))
    actor = _net(D, H1, H2, A, 3)
    with torch.no_grad():
        actor[4].weight.zero_(); actor[4].bias.zero_()
    q = types.SimpleNamespace(**vars(p))
    q.log_std = np.zeros(A, np.float32)
    got = _run_act(q, nets=(actor.to(_dev()), p.critic.to(_dev())))
    z = lr.noise(p.kw["seed"], p.kw["round_"], np.arange(rows), A)
    assert (got["mu"] == 0).all() and _same_bits(got["action"], z.astype(np.float32))
    zz = got["action"].astype(np.float64).ravel()
    want_logp = lr.act(**dict(p.kw, actor=[w.detach().cpu().numpy() for w in _params(actor)], log_std=q.log_std))["logp"]
    assert np.abs(got["logp"] - want_logp).max() < 1e-3 * np.abs(want_logp).max()
    print(f"act's draws: {zz.size} draws, mean {zz.mean():.5f} variance {zz.var():.5f} max |z| {np.abs(zz).max():.4f}")
    assert zz.size == 100_000 and abs(zz.mean()) < 0.02 and 0.97 <= zz.var() <= 1.03 and np.abs(zz).max() <= 6.0


# ---- a real environment ------------------------------------------------------------------------------------------------
def _piano_env(n_envs=5):
    from test_tasks_host import _get_test_midi
    from robopianist_amd.suite import environment
    from robopianist_amd.suite.tasks import SelfActuatedPiano
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        task = SelfActuatedPiano(midi=_get_test_midi(dt=0.01), n_steps_lookahead=1, control_timestep=0.01)
        return environment.Environment(task, n_envs=n_envs, precision=64)


def _snapshot(rollout):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in rollout.items()}


def _same_rollout(a, b):
    return [k for k in a if not _same_bits(a[k], b[k])]


def test_collect_on_the_self_actuated_piano():
    E, T = 5, 9
    env_a, env_b = _piano_env(E), _piano_env(E)
    kw = dict(hidden=(32, 16), horizon=T, seed=21, init_log_std=0.0)
    ppo_a, ppo_c = learning.PPO(env_a, **kw), learning.PPO(env_b, **kw)
    r1 = _snapshot(ppo_a.collect())
    # reproducible: another PPO of the same seed on another env in the same state
    assert _same_rollout(r1, _snapshot(ppo_c.collect())) == []
    st = r1["step_type"]
    assert ((st == L).sum(0) >= 2).all(), st.T.tolist()            # every env crosses at least two episode ends
    assert np.array_equal(r1["valid"] == 0, st[:T] == L) and (st[0] == F).all()
    assert _same_bits(r1["env_action"], np.fmin(np.fmax(r1["action"], -1), 1).astype(np.float64))
    assert np.isfinite(r1["adv"]).all() and np.isfinite(r1["logp"]).all()
    w = lr.gae(r1["reward"], r1["discount"], st, r1["value"], ppo_a.gamma, ppo_a.lam)
    assert _same_bits(r1["adv"], w[0]) and _same_bits(r1["ret"], w[1]) and _same_bits(r1["valid"], w[2])
    # the collector does not disturb the env: a second env stepped with the recorded actions sees the stored TimeSteps
    keys, D = ppo_a.observation_keys, ppo_a.D
    stats, slot = lr.new_stats(E), _slot(E, D)
    ts = env_b.reset()
    for t in range(T + 1):
        torch.cuda.synchronize()
        host = lambda x: None if x is None else x.cpu().numpy()
        lr.pack([host(ts.observation[k]) for k in keys], host(ts.step_type), host(ts.reward), host(ts.discount), slot, stats)
        for k in ("obs", "reward", "discount", "step_type"):
            assert _same_bits(slot[k], r1[k][t]), (k, t)
        if t < T:
            ts = env_b.step_canonical(_up(r1["env_action"][t]), ppo_a._bounds, False)
    got = ppo_a.episode_stats()
    n = int(stats["done_count"].sum())
    assert got["episodes"] == n >= 2 * E
    assert abs(got["mean_return"] - stats["done_return"].sum() / n) <= 1e-12 * abs(stats["done_return"]).sum()
    assert got["mean_length"] == stats["done_len"].sum() / n
    assert ppo_a.episode_stats()["episodes"] == 0                   # (read and reset)
    # resume: the learner's and the env's state_dict into the other pair; both continue with the same rollout
    ppo_a.update(); ppo_a.update_normalizer()
    ppo_b = learning.PPO(env_b, **dict(kw, seed=99))
    ppo_b.load_state_dict(ppo_a.state_dict())
    env_b.load_state_dict(env_a.state_dict())
    r2a, r2b = _snapshot(ppo_a.collect()), _snapshot(ppo_b.collect())
    assert _same_rollout(r2a, r2b) == []
    assert _same_bits(r2a["obs"][0], r1["obs"][T]) and not np.array_equal(r2a["action"], r1["action"])
    assert ppo_a.normalizer[0] == T * E and bool((ppo_a.normalizer[4] != 1).any())
    # evaluation: the mean action, clamped
    act = ppo_a.act(ts.observation, deterministic=True)
    torch.cuda.synchronize()
    assert tuple(act.shape) == (E, ppo_a.A) and act.dtype == torch.float64 and float(act.abs().max()) <= 1.0


def test_train_on_the_shadow_hands():
    from robopianist_amd import suite
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", n_envs=2, seed=3,
                         task_kwargs=dict(trim_silence=True, gravity_compensation=True, primitive_fingertip_collisions=True,
                                          n_steps_lookahead=2))
    ppo = learning.PPO(env, hidden=(64, 64), horizon=2, epochs=1, minibatches=1, seed=1)
    spec = env.observation_spec()
    assert ppo.D == sum(int(np.prod(s.shape)) for s in spec.values()) and ppo.A == env.action_spec().shape[0]
    log = ppo.train(1)
    r = _snapshot(ppo.rollout())
    assert all(np.isfinite(v).all() for v in r.values()) and log[0]["batch"] == 4
    assert all(np.isfinite(v) for k, v in log[0].items() if k not in ("mean_return", "mean_length")), log
    assert all(bool(torch.isfinite(p).all()) for p in ppo.actor.parameters())
    assert int(env.physics.warn.max()) == 0


# ---- it learns ---------------------------------------------------------------------------------------------------------
class _ToyEnv:
    """A dm_env-style batch in torch: the observation is 8 iid normals, the reward -mean((clamp(a) - obs[:2] / 2)^2) of
    the observation the action answered; episodes of 5 steps end by termination and a FIRST follows."""

    def __init__(self, E, seed):
        self.n_envs = E
        self.physics = types.SimpleNamespace(device=_dev(), dtype=torch.float32)
        self._gen = torch.Generator(device=_dev()).manual_seed(seed)
        self._obs = None
        self._age = torch.zeros(E, dtype=torch.int32, device=_dev())
        self._needs_reset = torch.ones(E, dtype=torch.bool, device=_dev())

    def observation_spec(self):
        return {"x": specs.Array((8,), np.float32)}

    def action_spec(self):
        return specs.BoundedArray((2,), np.float32, -1.0, 1.0)

    def _draw(self):
        return torch.randn(self.n_envs, 8, generator=self._gen, device=_dev())

    def reset(self):
        self._obs = self._draw()
        self._age.zero_(); self._needs_reset.zero_()
        return TimeStep(torch.zeros(self.n_envs, dtype=torch.int32, device=_dev()), None, None, {"x": self._obs})

    def step_canonical(self, action, bounds, clip=False):
        lo, rng = bounds
        a = lo + (action + 1.0) * 0.5 * rng
        resetting = self._needs_reset.clone()
        reward = -((a - 0.5 * self._obs[:, :2]) ** 2).mean(1)
        self._age = torch.where(resetting, torch.zeros_like(self._age), self._age + 1)
        last = self._age >= 5
        st = torch.where(last, 2, 1).to(torch.int32)
        st = torch.where(resetting, torch.zeros_like(st), st)
        reward = torch.where(resetting, torch.zeros_like(reward), reward).contiguous()
        discount = torch.where(last & ~resetting, 0.0, 1.0).to(torch.float32).contiguous()
        self._needs_reset = last & ~resetting
        self._obs = self._draw()
        return TimeStep(st, reward, discount, {"x": self._obs})


def test_ppo_learns_a_toy_task():
    """The mean reward of the last 5 of 40 updates is at least half-way from that of the first 5 to the optimum 0."""
    torch.manual_seed(0)
    env = _ToyEnv(256, seed=1)
    ppo = learning.PPO(env, hidden=(32, 32), horizon=8, lr=3e-3, gamma=0.9, seed=2)
    log = ppo.train(40)
    curve = [s["mean_reward"] for s in log]
    first5, last5 = float(np.mean(curve[:5])), float(np.mean(curve[-5:]))
    print(f"toy task: mean reward {first5:.4f} (first 5 updates) -> {last5:.4f} (last 5); ratio {last5 / first5:.3f}; "
          f"curve {[round(c, 3) for c in curve[::5]]}")
    assert first5 < -0.1 and last5 >= 0.5 * first5
    assert all(s["batch"] > 0 for s in log) and log[-1]["episodes"] > 0
