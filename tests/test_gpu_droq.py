"""GPU tests of the DroQ target kernel (include/learn/rp_droq.h) and of droq.DroQ.

The target is compared with the float64 twin (tests/droq_reference.py) under the bar of test_gpu_learn.py and
test_gpu_offpolicy.py: 8 times the error of a float32 numpy restatement of the same formulae on the same inputs,
computed by the test.  The dropout masks are integers and the same in the kernel and in both restatements, so the three
differ only by float32 rounding in another order.  The cases and their seeds are droq_cases's; test_droq_host.py checks
on the CPU that they are well conditioned (a second restatement in another order within 4 times the first one's error).

Measured on an MI355X (profiles/droq_gpu_tests.txt), kernel error | float32 restatement error against the float64 twin,
four critics (q: the worst of the four critics' own values by ratio):
    (rows, D, H1, H2, A, p)             y                   q_min               q
    ( 5,   1,  16,  16,   1, 0.5 )  6.48e-08 | 1.26e-07  7.52e-08 | 7.52e-08  1.86e-07 | 1.27e-07
    (17,  63,  48,  16,  45, 0.5 )  2.13e-07 | 1.67e-07  2.90e-07 | 1.81e-07  1.82e-07 | 8.85e-08
    (33, 255, 256, 256,  45, 0.01)  2.71e-07 | 3.04e-07  3.54e-07 | 3.24e-07  6.08e-07 | 4.88e-07
    (35, 300,  64,  64, 128, 0.25)  2.61e-07 | 3.10e-07  4.90e-07 | 3.70e-07  4.90e-07 | 3.70e-07
(the restatement's error was computed on the machine that ran the test; the bar is 8 times it; over all lines of the run
the ratio lies between 0.5 and 2.6).  Over the wide cases (droq_cases.WIDE_CASES: full tiles, D + A = 16 and 64, H1 < H2,
16 <-> 256; profiles/droq_wide_gpu_tests.txt) the worst ratio per line lies between 1.2 and 3.5 (the 3.5: q_min 6.27e-07 |
1.77e-07 of (64, 44, 16, 256, 20, 0.25) without dropout, three critics), in the rows [1024, 1040) of a batch of 1040 at 1.8
without dropout and 1.6 with it.  On the piano the three ranges' y had errors 3.61e-06, 4.54e-06 and 2.93e-06, each
equal to its restatement's.  The toy task went from a mean reward of -0.3738 over the first 5 rounds to -0.0414 over the
last 5 of 40 (ratio 0.111; every fifth round: -0.621, -0.107, -0.082, -0.062, -0.059, -0.057, -0.052, -0.041); its
hyper-parameters (TOY) were fixed once, before that run, from a CPU restatement of the same algorithm in torch over
three seeds, which gave the ratios 0.125, 0.116 and 0.118.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import droq_cases as dc  # noqa: E402
import droq_reference as dr  # noqa: E402
import sac_reference as sr  # noqa: E402
from test_gpu_offpolicy import POISON, _ToyEnv, _dev, _differing, _piano_env, _ranges, _same_bits, _snapshot, _stream, _up  # noqa: E402
from robopianist_amd import droq  # noqa: E402

pytestmark = pytest.mark.gpu


def _run_target(p, n, mode="on", first=0, count=None, round_=dc.ROUND, kw=None):
    """The target of the first n critics of case p (`kw`: its inputs, where they are not p.kw: a batch of any length)."""
    _, D, H1, H2, A, _ = p.case
    kw = p.kw if kw is None else kw
    rows = len(kw["next_obs"])
    dev = _dev()
    d = {k: _up(kw[k]) for k in ("next_obs", "action", "logp", "reward", "discount", "mean", "inv_std")}
    log_alpha = _up(np.array([kw["log_alpha"]], np.float32))
    out = {"y": torch.full((rows,), POISON, device=dev), "q_min": torch.full((rows,), POISON, device=dev),
           "q": torch.full((n, rows), POISON, device=dev)}
    drop = p.drop[mode]
    droq.target(d["next_obs"].data_ptr(), d["action"].data_ptr(), d["logp"].data_ptr(), d["reward"].data_ptr(),
                d["discount"].data_ptr(), d["mean"].data_ptr(), d["inv_std"].data_ptr(), dc.CLIP, dc.GAMMA,
                log_alpha.data_ptr(), [droq.critic_entry(dc.params(c.to(dev))) for c in p.critics[:n]], out["y"].data_ptr(),
                D, H1, H2, A, rows, q_min=out["q_min"].data_ptr(), q=out["q"].data_ptr(), threshold=drop["threshold"],
                keep_scale=drop["keep_scale"], ln_eps=dc.LN_EPS, seed=dc.SEED, round_=round_, row_first=first,
                row_count=count, hip_stream=_stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _within(got, ref, err32, label):
    pairs = {k: (float(np.abs(got[k].astype(np.float64) - ref[k]).max()), err32[k]) for k in ref}
    worst = max((e / b if b > 0 else (np.inf if e > 0 else 0.0)) for e, b in pairs.values())
    print(f"{label}: kernel error | float32 restatement error: " + ", ".join(f"{k} {e:.2e} | {b:.2e}" for k, (e, b) in pairs.items()) +
          f" (worst ratio: {worst:.2f})")
    for k, (e, b) in pairs.items():
        assert e <= 8 * b, (label, k, e, b)


@pytest.mark.parametrize("case", dc.ALL_CASES, ids=dc.case_id)
def test_target_equals_the_float64_twin_within_8_float32_restatement_errors(case):
    p = dc.problem(case)
    stop = p.kw["discount"] == 0
    assert stop.any()
    for n in dc.N_CRITICS:
        got = _run_target(p, n)
        _within(dc.flat(got), p.ref["on", n], p.err32["on", n], f"target {case} critics {n}")
        assert _same_bits(got["y"][stop], p.kw["reward"][stop])
        qm = got["q"][0]
        for q in got["q"][1:]:
            qm = np.fmin(qm, q)
        assert _same_bits(got["q_min"], qm) and np.isfinite(got["q"]).all()


@pytest.mark.parametrize("case", dc.ALL_CASES, ids=dc.case_id)
def test_target_without_dropout_is_torchs_eval_forward(case):
    p = dc.problem(case)
    dev = _dev()
    for n in (1, 3):
        got = dc.flat(_run_target(p, n, mode="off"))
        _within(got, p.ref["off", n], p.err32["off", n], f"target {case} critics {n} dropout off")
        with torch.no_grad():
            xn = torch.clamp((_up(p.kw["next_obs"]) - _up(p.kw["mean"])) * _up(p.kw["inv_std"]), -dc.CLIP, dc.CLIP)
            xa = torch.cat([xn, _up(p.kw["action"])], dim=1)
            t_q = torch.stack([c.to(dev).eval()(xa)[:, 0] for c in p.critics[:n]])
            want = dict({"q_min": t_q.min(0).values.cpu().numpy()}, **{f"q{i}": q.cpu().numpy() for i, q in enumerate(t_q)})
        for c in p.critics[:n]:
            c.train()
        pairs = {k: (float(np.abs(got[k].astype(np.float64) - w).max()), p.err32["off", n][k]) for k, w in want.items()}
        print(f"target {case} critics {n} dropout off: against torch's eval() forward on the GPU | float32 restatement "
              "error: " + ", ".join(f"{k} {e:.2e} | {b:.2e}" for k, (e, b) in pairs.items()))
        for k, (e, b) in pairs.items():
            assert e <= 8 * b, (case, n, k, e, b)


@pytest.mark.parametrize("case", dc.CASES[1:3], ids=dc.case_id)
def test_target_row_ranges(case):
    p = dc.problem(case)
    rows = case[0]
    full = _run_target(p, 2)
    for first, count in _ranges(rows):
        part = _run_target(p, 2, first=first, count=count)
        inside = np.zeros(rows, bool); inside[first:first + count] = True
        for k in ("y", "q_min"):
            assert _same_bits(part[k][inside], full[k][inside]) and (part[k][~inside] == POISON).all(), (k, first, count)
        assert _same_bits(part["q"][:, inside], full["q"][:, inside]) and (part["q"][:, ~inside] == POISON).all()


DEEP_B, DEEP_FIRST = 1040, 1024


def deep(kw, keys, rows):
    """`kw` with the per-row arrays `keys` moved to the rows [DEEP_FIRST, DEEP_FIRST + rows) of a batch of DEEP_B rows; every
    other row is NaN."""
    assert DEEP_FIRST + rows == DEEP_B
    out = dict(kw)
    for k in keys:
        out[k] = np.full((DEEP_B,) + kw[k].shape[1:], np.nan, np.float32)
        out[k][DEEP_FIRST:] = kw[k]
    return out


def test_target_deep_in_a_batch_differs_by_addresses_and_masks_only():
    """A range at row 1024 of 1040: the tile partition is relative to row_first, so without dropout nothing but addresses
    differs from the 16-row call; with dropout the masks are keyed by the batch row, so the values differ and are the
    twin's at that row_first."""
    case = dc.WIDE_CASES[1]
    p, rows, n = dc.problem(case), case[0], 2
    kw = deep(p.kw, ("next_obs", "action", "logp", "reward", "discount"), rows)
    inside = np.zeros(DEEP_B, bool); inside[DEEP_FIRST:] = True
    live = p.kw["discount"] != 0
    for mode in ("off", "on"):
        compact = _run_target(p, n, mode)
        got = _run_target(p, n, mode, first=DEEP_FIRST, count=rows, kw=kw)
        assert all((got[k][..., ~inside] == POISON).all() and np.isfinite(got[k][..., inside]).all() for k in got), mode
        there = {k: v[..., inside] for k, v in got.items()}
        if mode == "off":
            assert [k for k in there if not _same_bits(there[k], compact[k])] == []
        else:
            assert not np.array_equal(there["q"], compact["q"]) and not np.array_equal(there["q_min"], compact["q_min"])
            assert not np.array_equal(there["y"][live], compact["y"][live])
            assert _same_bits(there["y"][~live], compact["y"][~live])
        run = lambda **o: dc.flat(dr.target(critics=[dc.host(c) for c in p.critics[:n]], **kw, **p.drop[mode],
                                            row_first=DEEP_FIRST, row_count=rows, **o))
        ref = run(dtype=np.float64)
        _within(dc.flat(there), ref, dc.errors(run(dtype=np.float32), ref), f"target {case} rows [{DEEP_FIRST}, {DEEP_B}) dropout {mode}")


@pytest.mark.parametrize("case", [dc.CASES[0], dc.CASES[3]], ids=dc.case_id)
def test_target_is_deterministic_and_the_round_changes_it(case):
    p = dc.problem(case)
    a, b = _run_target(p, 2), _run_target(p, 2)
    assert all(_same_bits(a[k], b[k]) for k in a)
    other = _run_target(p, 2, round_=dc.ROUND + 1)
    live = p.kw["discount"] != 0
    assert not np.array_equal(other["y"][live], a["y"][live]) and not np.array_equal(other["q"], a["q"])
    assert _same_bits(other["y"][~live], a["y"][~live])


# ---- a real environment ------------------------------------------------------------------------------------------------
def _host_params(nets):
    torch.cuda.synchronize()
    return [[t.detach().cpu().numpy().copy() for t in dc.params(net)] for net in nets]


def test_droq_on_the_self_actuated_piano():
    E, C, B, utd, tau = 5, 4, 16, 3, 0.25
    env_a, env_b = _piano_env(E), _piano_env(E)
    kw = dict(hidden=(32, 16), n_critics=2, capacity=C, batch_size=B, lr=1e-3, tau=tau, seed=21, utd=utd, dropout=0.5)
    d_a, d_b = droq.DroQ(env_a, **kw), droq.DroQ(env_b, **kw)
    d_a.collect(6); d_b.collect(6)
    assert _differing(_snapshot(d_a), _snapshot(d_b)) == [] and d_a.n_written == 7
    params = list(d_a.actor.parameters()) + [p for c in d_a.critics for p in c.parameters()] + [d_a.log_alpha]
    before = [p.detach().clone() for p in params]
    # the target weights as they are before each range's launch, and both sets after each critic step
    before_range, after_step = [], []
    target_range, critic_step = d_a.target_range, d_a.critic_step

    def hooked_target_range(u):
        before_range.append(_host_params(d_a.targets))
        return target_range(u)

    def hooked_critic_step(batch):
        out = critic_step(batch)
        after_step.append((_host_params(d_a.critics), _host_params(d_a.targets)))
        return out

    d_a.target_range, d_a.critic_step = hooked_target_range, hooked_critic_step
    round_, log_alpha = d_a._round, float(d_a.log_alpha.detach().cpu()[0])
    ring = _snapshot(d_a)
    stats = d_a.update(1)
    del d_a.target_range, d_a.critic_step
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in stats.values()), stats
    assert d_a._round == round_ + 1 and len(before_range) == len(after_step) == utd
    for b, a in zip(before, params):
        assert bool((a != b).any()) and bool(torch.isfinite(a).all())
    assert len(params) == 6 + 2 * 10 + 1
    # three successive tau steps, each towards the critics as they were after that critic step
    for u in range(utd):
        crit, targ = after_step[u]
        for net_b, net_c, net_t in zip(before_range[u], crit, targ):
            for tb, c, ta in zip(net_b, net_c, net_t):
                np.testing.assert_allclose(ta, tb + np.float32(tau) * (c - tb), rtol=1e-5, atol=1e-7)
                assert not np.array_equal(ta, tb)
        if u + 1 < utd:
            assert all(_same_bits(x, y) for nx, ny in zip(targ, before_range[u + 1]) for x, y in zip(nx, ny))
    assert all(_same_bits(x, y) for nx, ny in zip(after_step[-1][1], _host_params(d_a.targets)) for x, y in zip(nx, ny))
    # the utd x B rows are the twin's, drawn in one launch from the ring as it stood
    rows = {k: getattr(d_a, "_u_" + k).cpu().numpy() for k in ("obs", "next", "action", "reward", "discount", "mask",
                                                               "next_action", "next_logp", "y")}
    want = sr.sample(ring, d_a.n_written, utd * B, d_a.seed, round_)
    for k, w in (("obs", "obs"), ("next", "next_obs"), ("action", "action"), ("reward", "reward"), ("discount", "discount"),
                 ("mask", "mask")):
        assert _same_bits(rows[k], want[w]), k
    assert rows["mask"].sum() >= 1 and all(np.isfinite(v).all() for v in rows.values())
    batch = {k: v.cpu().numpy() for k, v in d_a.minibatch().items()}
    assert _same_bits(batch["y"], rows["y"][(utd - 1) * B:]) and _same_bits(batch["obs"], rows["obs"][(utd - 1) * B:])
    # y of each range: the twin on the target weights of before that range's Polyak step
    mean, inv_std = d_a.normalizer[3].cpu().numpy(), d_a.normalizer[4].cpu().numpy()
    for u in range(utd):
        tkw = dict(next_obs=rows["next"], action=rows["next_action"], logp=rows["next_logp"], reward=rows["reward"],
                   discount=rows["discount"], mean=mean, inv_std=inv_std, clip=d_a.obs_clip, gamma=d_a.gamma,
                   log_alpha=np.float32(log_alpha), critics=before_range[u], threshold=droq.drop_threshold(0.5),
                   keep_scale=2.0, ln_eps=d_a.ln_eps, seed=d_a.seed, round_=round_, row_first=u * B, row_count=B)
        ref, f32 = dr.target(dtype=np.float64, **tkw), dr.target(dtype=np.float32, **tkw)
        e = float(np.abs(rows["y"][u * B:(u + 1) * B].astype(np.float64) - ref["y"]).max())
        bar = float(np.abs(f32["y"].astype(np.float64) - ref["y"]).max())
        print(f"DroQ update, range {u}: kernel error | float32 restatement error: y {e:.2e} | {bar:.2e}")
        assert e <= 8 * bar, (u, e, bar)
    # resume: the learner's and the env's state_dict into the other pair; both continue with the same TimeSteps
    d_b.load_state_dict(d_a.state_dict())
    env_b.load_state_dict(env_a.state_dict())
    d_a.collect(3); d_b.collect(3)
    ra, rb = _snapshot(d_a), _snapshot(d_b)
    new = [m % C for m in range(d_a.n_written - 3, d_a.n_written)]
    for k in ra:
        assert _same_bits(ra[k][new], rb[k][new]), k
    assert d_b.n_written == d_a.n_written == 10 and not np.array_equal(ra["obs"], ring["obs"])
    assert all(torch.equal(x, y) for x, y in zip(d_a.normalizer[1:], d_b.normalizer[1:]))
    with pytest.raises(ValueError, match="written with utd"):
        droq.DroQ(env_b, **dict(kw, utd=2)).load_state_dict(d_a.state_dict())


# ---- it learns ---------------------------------------------------------------------------------------------------------
TOY = dict(rounds=40, steps_per_round=8, grad_steps=4,
           droq=dict(hidden=(32, 32), capacity=32, batch_size=256, lr=1e-2, gamma=0.9, tau=0.05, init_alpha=0.1, seed=2,
                     utd=4, dropout=0.01))


def test_droq_learns_a_toy_task():
    """PPO's criterion unchanged: the mean reward of the last 5 of 40 rounds is at least half-way from that of the
    first 5 to the optimum 0."""
    torch.manual_seed(0)
    env = _ToyEnv(256, seed=1)
    learner = droq.DroQ(env, **TOY["droq"])
    log = learner.train(TOY["rounds"], TOY["steps_per_round"], TOY["grad_steps"])
    curve = [s["mean_reward"] for s in log]
    first5, last5 = float(np.mean(curve[:5])), float(np.mean(curve[-5:]))
    print(f"toy task: mean reward {first5:.4f} (first 5 rounds) -> {last5:.4f} (last 5); ratio {last5 / first5:.3f}; "
          f"alpha {log[-1]['alpha']:.4f}; curve {[round(c, 3) for c in curve[::5]]}")
    assert first5 < -0.1 and last5 >= 0.5 * first5
    assert all(np.isfinite(s["critic_loss"]) for s in log) and log[-1]["episodes"] > 0
