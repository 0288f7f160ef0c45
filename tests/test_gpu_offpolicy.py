"""GPU tests of the off-policy learner kernels (include/learn/rp_sac.h) and of offpolicy.SAC.

sample is compared with the numpy twin (tests/sac_reference.py) bit for bit.  act and target are compared with the
float64 twin under the bar of test_gpu_learn.py: 8 times the error of a float32 numpy restatement of the same formulae
on the same inputs, computed by the test (the kernels differ from the twin only by float32 rounding in another order
and by another tanhf / expf / log1pf).  The error pairs of a run are in profiles/sac_gpu_tests.txt.

The sampler's step types are staggered 6-slot episodes, (FIRST, 4 x MID, LAST)[(m + e) % 6] for TimeStep m of env e.
With seed (7 << 32) | 11 and round 3 on the (5, 65, 63, 45, 13) ring the twin finds 216 of 260 candidates valid; at
B = 8192 all 216 are drawn and nothing else, 7 rows are masked; at B = 257, 40 rows need a retry and none is masked.

Measured on an MI355X (profiles/sac_gpu_tests.txt), kernel error | float32 restatement error against the float64 twin:
    (rows, D, H1, H2, A)           action              pre                 logp                y (3 critics)
    ( 1,    1,  16,  16,   1)  2.74e-08 | 3.22e-08  5.02e-08 | 6.90e-08  8.43e-09 | 1.28e-07  1.09e-08 | 1.09e-08
    (17,   63,  48,  16,  45)  1.57e-07 | 1.29e-07  1.72e-06 | 1.33e-06  9.04e-06 | 8.02e-06  4.82e-07 | 9.61e-07
    (65, 1068, 256, 256,  89)  4.57e-07 | 4.24e-07  1.94e-06 | 2.07e-06  4.41e-05 | 4.99e-05  1.84e-06 | 1.84e-06
    (70, 1136,  64,  64, 128)  3.53e-07 | 4.71e-07  1.48e-06 | 2.14e-06  8.41e-05 | 8.41e-05  1.68e-06 | 1.49e-06
(the restatement's error was computed on the machine that ran the test; the bar is 8 times it).  The toy task went from
a mean reward of -0.5220 over the first 5 rounds to -0.0159 over the last 5 of 40 (ratio 0.030; every fifth round:
-0.621, -0.33, -0.098, -0.055, -0.029, -0.022, -0.015, -0.016); its hyper-parameters were fixed once, from a CPU
restatement of the same algorithm in torch over three seeds, before that run.
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
import sac_reference as sr  # noqa: E402
from robopianist_amd import learning, offpolicy  # noqa: E402
from robopianist_amd.suite import specs  # noqa: E402
from robopianist_amd.suite.specs import TimeStep  # noqa: E402

pytestmark = pytest.mark.gpu

F, M, L = sr.FIRST, sr.MID, sr.LAST
POISON = -777.0
SEED, ROUND = (7 << 32) | 11, 3


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _up(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=_dev())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _ranges(E):
    return [r for r in dict.fromkeys([(0, E), (1, E - 2), (E - 1, 1)]) if r[1] >= 0 and r[0] + r[1] <= E]


# ---- sample ------------------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(2, 1, 1, 1, 2, 5), (4, 3, 5, 3, 3, 70), (5, 65, 63, 45, 13, 257), (3, 2, 1130, 45, 9, 33)]
STAGGERED = lambda m, e: (F, M, M, M, M, L)[(m + e) % 6]   # noqa: E731


@functools.lru_cache(maxsize=None)
def _ring(C, E, D, A, n_written, pattern="staggered"):
    rng = np.random.default_rng(C + E + D + A)
    ring = {"obs": rng.normal(size=(C, E, D)).astype(np.float32), "action": rng.uniform(-1, 1, (C, E, A)).astype(np.float32),
            "reward": rng.normal(size=(C, E)).astype(np.float32), "discount": rng.uniform(size=(C, E)).astype(np.float32),
            "step_type": np.full((C, E), {"staggered": M, "last": L, "mid": M}[pattern], np.int32)}
    if pattern == "staggered":
        for m in range(max(0, n_written - C), n_written):
            ring["step_type"][m % C] = [STAGGERED(m, e) for e in range(E)]
    return ring


_OUT = (("obs", "D", np.float32), ("next_obs", "D", np.float32), ("action", "A", np.float32), ("reward", 0, np.float32),
        ("discount", 0, np.float32), ("mask", 0, np.float32), ("index", 0, np.int32))


def _poisoned(B, D, A):
    return {k: np.full((B, {"D": D, "A": A}[w]) if w else (B,), POISON, dt) for k, w, dt in _OUT}


def _run_sample(ring, n_written, B, seed=SEED, round_=ROUND, first=0, count=None, index=True):
    C, E, D = ring["obs"].shape
    A = ring["action"].shape[2]
    d_ring = {k: _up(v) for k, v in ring.items()}
    out = {k: _up(v) for k, v in _poisoned(B, D, A).items()}
    offpolicy.sample(d_ring["obs"].data_ptr(), d_ring["action"].data_ptr(), d_ring["reward"].data_ptr(),
                     d_ring["discount"].data_ptr(), d_ring["step_type"].data_ptr(), out["obs"].data_ptr(),
                     out["next_obs"].data_ptr(), out["action"].data_ptr(), out["reward"].data_ptr(),
                     out["discount"].data_ptr(), out["mask"].data_ptr(), n_written, C, E, D, A, B,
                     index=out["index"].data_ptr() if index else None, seed=seed, round_=round_, row_first=first,
                     row_count=count, hip_stream=_stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _equals_twin(got, want):
    return [k for k, _, _ in _OUT if not _same_bits(got[k], want[k])]


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sample_equals_the_twin_bit_for_bit(case):
    C, E, D, A, n_written, B = case
    ring = _ring(C, E, D, A, n_written)
    want = sr.sample(ring, n_written, B, SEED, ROUND)
    got = _run_sample(ring, n_written, B)
    assert _equals_twin(got, want) == []
    valid = sr.valid_transitions(ring["step_type"], n_written)
    print(f"sample {case}: {int(valid.sum())} of {valid.size} candidates valid, {int((want['tries'] > 1).sum())} rows "
          f"retried, {int((want['mask'] == 0).sum())} masked")
    if case == SAMPLE_CASES[2]:
        assert (want["tries"][want["mask"] == 1] > 1).any()               # a retried row is part of the comparison
        newest = (n_written - 1) % C
        assert (got["index"][got["mask"] == 1] // E != newest).all()
    # a row sub-range leaves the other rows poisoned; no index array is accepted
    for first, count in _ranges(B)[1:]:
        part = _run_sample(ring, n_written, B, first=first, count=count, index=False)
        inside = np.zeros(B, bool); inside[first:first + count] = True
        for k, _, _ in _OUT[:-1]:
            assert _same_bits(part[k][inside], want[k][inside]), (k, first, count)
            assert (part[k][~inside] == POISON).all(), (k, first, count)
        assert (part["index"] == int(POISON)).all()
    # the same arguments give the same bits twice; another round gives other indices
    assert _equals_twin(_run_sample(ring, n_written, B), got) == []
    if valid.sum() > 1:
        assert not np.array_equal(_run_sample(ring, n_written, B, round_=ROUND + 1)["index"], got["index"])


def test_sample_8192_rows_draw_every_valid_transition_and_mask_under_one_percent():
    C, E, D, A, n_written, _ = SAMPLE_CASES[2]
    B = 8192
    ring = _ring(C, E, D, A, n_written)
    want = sr.sample(ring, n_written, B, SEED, ROUND)
    masked = want["mask"] == 0
    assert masked.mean() <= 0.01
    valid = sr.valid_transitions(ring["step_type"], n_written)
    m = sr.candidates(n_written, C)
    ok = np.zeros((C, E), bool)
    ok[m % C] = valid
    assert set(want["index"][~masked].tolist()) == set(np.flatnonzero(ok.ravel()).tolist())
    got = _run_sample(ring, n_written, B)
    assert _equals_twin(got, want) == []
    for k in ("obs", "next_obs", "action", "reward", "discount"):
        assert (got[k][masked] == 0).all() and np.isfinite(got[k]).all()
    assert (got["index"][masked] == -1).all()


def test_sample_all_last_masks_every_row_and_all_mid_none():
    C, E, D, A, n_written, B = 4, 3, 5, 3, 11, 70
    got = _run_sample(_ring(C, E, D, A, n_written, "last"), n_written, B)
    assert (got["mask"] == 0).all() and (got["index"] == -1).all()
    assert all((got[k] == 0).all() for k in ("obs", "next_obs", "action", "reward", "discount"))
    ring = _ring(C, E, D, A, n_written, "mid")
    got = _run_sample(ring, n_written, B)
    assert (got["mask"] == 1).all() and _equals_twin(got, sr.sample(ring, n_written, B, SEED, ROUND)) == []


# ---- act and target ------------------------------------------------------------------------------------------------------
ACT_CASES = [(1, 1, 16, 16, 1), (15, 3, 16, 48, 3), (17, 63, 48, 16, 45), (33, 65, 256, 256, 89),
             (65, 1068, 256, 256, 89), (70, 1136, 64, 64, 128)]
BOUNDS = (-5.0, 2.0)


def _net(n_in, H1, H2, n_out, seed):
    """Weights drawn as nn.Linear draws them."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(n_in, H1), torch.nn.Tanh(), torch.nn.Linear(H1, H2), torch.nn.Tanh(),
                                   torch.nn.Linear(H2, n_out))


def _params(net):
    return [t for i in (0, 2, 4) for t in (net[i].weight, net[i].bias)]


def _host(net):
    return [p.detach().cpu().numpy() for p in _params(net)]


def _errors(f32, ref, keys):
    return {k: float(np.abs(f32[k].astype(np.float64) - ref[k]).max()) for k in keys}


@functools.lru_cache(maxsize=None)
def _act_problem(case):
    """The inputs of a case, the float64 twins of act and target, and the float32 restatement's errors -- computed once."""
    rows, D, H1, H2, A = case
    rng = np.random.default_rng(sum(case))
    actor = _net(D, H1, H2, 2 * A, 1 + rows)
    with torch.no_grad():   # every eleventh log-std head lies outside the bounds, above and below in turn
        for u in range(2, A, 11):
            actor[4].bias[A + u] += 9.0 if (u // 11) % 2 == 0 else -9.0
    critics = [_net(D + A, H1, H2, 1, 10 + i + rows) for i in range(3)]
    mean = rng.normal(size=D).astype(np.float32)
    inv_std = (1.0 / rng.uniform(0.5, 2.0, D)).astype(np.float32)
    obs = (mean + rng.normal(size=(rows, D)) * 2.0).astype(np.float32)
    obs.reshape(-1)[5::11] += 40.0                                    # every eleventh normalised entry clips at 5
    kw = dict(obs=obs, mean=mean, inv_std=inv_std, clip=5.0, actor=_host(actor), log_std_bounds=BOUNDS, seed=SEED,
              round_=ROUND)
    ref, f32 = sr.act(dtype=np.float64, **kw), sr.act(dtype=np.float32, **kw)
    det, det32 = sr.act(dtype=np.float64, deterministic=True, **kw), sr.act(dtype=np.float32, deterministic=True, **kw)
    # the target's inputs: the float32 restatement's own action and logp (what a kernel would have handed on)
    tkw = dict(next_obs=obs, action=f32["action"], logp=f32["logp"], reward=rng.normal(size=rows).astype(np.float32),
               discount=np.where(np.arange(rows) % 3 == 1, 0.0, rng.uniform(0.5, 1.0, rows)).astype(np.float32), mean=mean,
               inv_std=inv_std, clip=5.0, gamma=0.97, log_alpha=np.float32(-0.7))
    tref = {n: sr.target(critics=[_host(c) for c in critics[:n]], dtype=np.float64, **tkw) for n in (1, 2, 3)}
    t32 = {n: sr.target(critics=[_host(c) for c in critics[:n]], dtype=np.float32, **tkw) for n in (1, 2, 3)}
    return types.SimpleNamespace(
        case=case, actor=actor, critics=critics, kw=kw, tkw=tkw, ref=ref, det=det, tref=tref,
        err32=_errors(f32, ref, ("action", "pre", "logp")), det_err32=_errors(det32, det, ("action", "pre")),
        terr32={n: _errors(t32[n], tref[n], ("y", "q_min")) for n in (1, 2, 3)},
        clamped=float(((ref["log_std"] == BOUNDS[0]) | (ref["log_std"] == BOUNDS[1])).mean()))


def _run_act(p, precision=64, deterministic=False, first=0, count=None, round_=ROUND, env_action=True):
    rows, D, H1, H2, A = p.case
    dev = _dev()
    edt = torch.float32 if precision == 32 else torch.float64
    out = {"action": torch.full((rows, A), POISON, device=dev), "logp": torch.full((rows,), POISON, device=dev),
           "pre": torch.full((rows, A), POISON, device=dev),
           "env_action": torch.full((rows, A), POISON, device=dev, dtype=edt)}
    d = {k: _up(p.kw[k]) for k in ("obs", "mean", "inv_std")}
    offpolicy.act(d["obs"].data_ptr(), d["mean"].data_ptr(), d["inv_std"].data_ptr(), 5.0,
                  learning.mlp_table(_params(p.actor.to(dev))), D, H1, H2, A, rows, log_std_bounds=BOUNDS,
                  action=out["action"].data_ptr(), logp=out["logp"].data_ptr(), pre=out["pre"].data_ptr(),
                  env_action=out["env_action"].data_ptr() if env_action else None, precision=precision,
                  deterministic=deterministic, seed=SEED, round_=round_, row_first=first, row_count=count,
                  hip_stream=_stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _within(got, ref, err32, keys, label):
    pairs = {k: (float(np.abs(got[k].astype(np.float64) - ref[k]).max()), err32[k]) for k in keys}
    line = f"{label}: kernel error | float32 restatement error: " + ", ".join(
        f"{k} {e:.2e} | {b:.2e}" for k, (e, b) in pairs.items())
    print(line)
    for k, (e, b) in pairs.items():
        assert e <= 8 * b, (label, k, e, b)


@pytest.mark.parametrize("case", ACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_act_equals_the_float64_twin_within_8_float32_restatement_errors(case):
    p = _act_problem(case)
    rows, D, H1, H2, A = case
    assert A < 3 or p.clamped > 0.01
    got = _run_act(p)
    _within(got, p.ref, p.err32, ("action", "pre", "logp"), f"act {case}")
    assert (np.abs(got["action"]) <= 1).all() and np.isfinite(got["logp"]).all()
    # the env's action is the stored action, exactly, in both precisions; without the array nothing else changes
    assert _same_bits(got["env_action"], got["action"].astype(np.float64))
    got32 = _run_act(p, precision=32)
    assert _same_bits(got32["env_action"], got32["action"])
    none = _run_act(p, env_action=False)
    assert (none["env_action"] == POISON).all()
    # the same arguments give the same bits twice
    for k in ("action", "logp", "pre"):
        assert _same_bits(got[k], got32[k]) and _same_bits(got[k], none[k]), k
    det = _run_act(p, deterministic=True)
    _within(det, p.det, p.det_err32, ("action", "pre"), f"act {case} deterministic")
    assert (det["logp"] == POISON).all() and _same_bits(det["env_action"], det["action"].astype(np.float64))
    other = _run_act(p, round_=ROUND + 1)
    assert not np.array_equal(other["action"], got["action"]) and not np.array_equal(other["logp"], got["logp"])


@pytest.mark.parametrize("case", [ACT_CASES[2], ACT_CASES[4]], ids=lambda c: "x".join(map(str, c)))
def test_act_row_ranges(case):
    p = _act_problem(case)
    rows = case[0]
    full = _run_act(p)
    for first, count in _ranges(rows):
        for det in (False, True):
            want = _run_act(p, deterministic=True) if det else full
            got = _run_act(p, first=first, count=count, deterministic=det)
            inside = np.zeros(rows, bool); inside[first:first + count] = True
            for k in ("action", "pre", "env_action") + (() if det else ("logp",)):
                assert _same_bits(got[k][inside], want[k][inside]), (k, first, count)
                assert (got[k][~inside] == POISON).all(), (k, first, count)


def _run_target(p, n, first=0, count=None):
    rows, D, H1, H2, A = p.case
    dev = _dev()
    d = {k: _up(p.tkw[k]) for k in ("next_obs", "action", "logp", "reward", "discount", "mean", "inv_std")}
    log_alpha = _up(np.array([p.tkw["log_alpha"]], np.float32))
    out = {"y": torch.full((rows,), POISON, device=dev), "q_min": torch.full((rows,), POISON, device=dev)}
    offpolicy.target(d["next_obs"].data_ptr(), d["action"].data_ptr(), d["logp"].data_ptr(), d["reward"].data_ptr(),
                     d["discount"].data_ptr(), d["mean"].data_ptr(), d["inv_std"].data_ptr(), 5.0, p.tkw["gamma"],
                     log_alpha.data_ptr(), [learning.mlp_table(_params(c.to(dev))) for c in p.critics[:n]],
                     out["y"].data_ptr(), D, H1, H2, A, rows, q_min=out["q_min"].data_ptr(), row_first=first,
                     row_count=count, hip_stream=_stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", ACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_target_equals_the_float64_twin_within_8_float32_restatement_errors(case):
    p = _act_problem(case)
    rows, D, H1, H2, A = case
    got = {}
    for n in (1, 2, 3):
        got[n] = _run_target(p, n)
        _within(got[n], p.tref[n], p.terr32[n], ("y", "q_min"), f"target {case} critics {n}")
        stop = p.tkw["discount"] == 0
        assert _same_bits(got[n]["y"][stop], p.tkw["reward"][stop]) and (stop.any() or rows < 2)
        # torch's own forward of the same modules on the GPU
        with torch.no_grad():
            xn = torch.clamp((_up(p.tkw["next_obs"]) - _up(p.tkw["mean"])) * _up(p.tkw["inv_std"]), -5.0, 5.0)
            xa = torch.cat([xn, _up(p.tkw["action"])], dim=1)
            t_q = torch.stack([c.to(_dev())(xa)[:, 0] for c in p.critics[:n]]).min(0).values.cpu().numpy()
        e_q = float(np.abs(got[n]["q_min"].astype(np.float64) - t_q).max())
        print(f"target {case} critics {n}: against torch's forward on the GPU: q_min {e_q:.2e}")
        assert e_q <= 8 * p.terr32[n]["q_min"]
    assert (got[2]["q_min"] <= got[1]["q_min"]).all() and (got[3]["q_min"] <= got[2]["q_min"]).all()
    for first, count in _ranges(rows)[1:]:
        part = _run_target(p, 2, first=first, count=count)
        inside = np.zeros(rows, bool); inside[first:first + count] = True
        for k in ("y", "q_min"):
            assert _same_bits(part[k][inside], got[2][k][inside]) and (part[k][~inside] == POISON).all(), (k, first, count)


# ---- a real environment ------------------------------------------------------------------------------------------------
def _piano_env(n_envs=5):
    from test_tasks_host import _get_test_midi
    from robopianist_amd.suite import environment
    from robopianist_amd.suite.tasks import SelfActuatedPiano
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        task = SelfActuatedPiano(midi=_get_test_midi(dt=0.01), n_steps_lookahead=1, control_timestep=0.01)
        return environment.Environment(task, n_envs=n_envs, precision=64)


def _snapshot(sac):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in sac.ring().items()}


def _differing(a, b):
    return [k for k in a if not _same_bits(a[k], b[k])]


def test_sac_on_the_self_actuated_piano():
    E, C, steps = 5, 4, 10
    env_a, env_b = _piano_env(E), _piano_env(E)
    kw = dict(hidden=(32, 16), n_critics=2, capacity=C, batch_size=16, lr=1e-3, tau=0.25, seed=21)
    sac_a, sac_b = offpolicy.SAC(env_a, **kw), offpolicy.SAC(env_b, **kw)
    snaps = []
    for _ in range(steps):   # one control step per call: the ring is looked at before it is written over
        sac_a.collect(1); sac_b.collect(1)
        snaps.append(_snapshot(sac_a))
        assert _differing(snaps[-1], _snapshot(sac_b)) == []           # two runs from the same state: the same bits
    assert sac_a.n_written == steps + 1 > 2 * C and sac_a.normalizer[0] == (steps + 1) * E
    # a second env stepped with the recorded actions returns the TimeSteps the slots hold
    keys, D = sac_a.observation_keys, sac_a.D
    host = lambda x: None if x is None else x.cpu().numpy()
    slot = {"obs": np.zeros((E, D), np.float32), "reward": np.zeros(E, np.float32), "discount": np.zeros(E, np.float32),
            "step_type": np.zeros(E, np.int32)}
    stats, seen = lr.new_stats(E), []
    ts = env_b.reset()
    for m in range(steps + 1):
        torch.cuda.synchronize()
        lr.pack([host(ts.observation[k]) for k in keys], host(ts.step_type), host(ts.reward), host(ts.discount), slot, stats)
        after = snaps[max(m - 1, 0)]                                   # the ring after TimeStep m was written
        for k in ("obs", "reward", "discount", "step_type"):
            assert _same_bits(after[k][m % C], slot[k]), (k, m)
        seen.append(slot["step_type"].copy())
        if m < steps:
            a = snaps[m]["action"][m % C]                              # decided at TimeStep m, in the call that wrote m + 1
            assert (np.abs(a) <= 1).all()
            ts = env_b.step_canonical(_up(a.astype(np.float64)), sac_a._bounds, False)
    seen = np.array(seen)
    assert (seen[0] == F).all() and ((seen == L).sum(0) >= 1).all(), seen.T.tolist()     # every env ends an episode
    got = sac_a.episode_stats()
    n = int(stats["done_count"].sum())
    assert got["episodes"] == n >= E and got["mean_length"] == stats["done_len"].sum() / n
    assert abs(got["mean_return"] - stats["done_return"].sum() / n) <= 1e-12 * abs(stats["done_return"]).sum()
    # one update: every parameter tensor changes, every target moves by tau towards its source, nothing is non-finite
    params = list(sac_a.actor.parameters()) + [p for c in sac_a.critics for p in c.parameters()] + [sac_a.log_alpha]
    before = [p.detach().clone() for p in params]
    t_before = [p.detach().clone() for t in sac_a.targets for p in t.parameters()]
    stats = sac_a.update(1)
    batch = {k: v.cpu().numpy() for k, v in sac_a.minibatch().items()}
    assert all(np.isfinite(v) for v in stats.values()), stats
    assert all(np.isfinite(v).all() for v in batch.values()) and batch["mask"].sum() >= 1
    for b, a in zip(before, params):
        assert bool((a != b).any()) and bool(torch.isfinite(a).all())
    src = [p.detach() for c in sac_a.critics for p in c.parameters()]
    for tb, ta, s in zip(t_before, [p for t in sac_a.targets for p in t.parameters()], src):
        assert torch.allclose(ta, tb + 0.25 * (s - tb), rtol=1e-5, atol=1e-7) and not torch.equal(ta, tb)
    # the minibatch is the twin's, drawn from the ring as it stands
    ring = _snapshot(sac_a)
    want = sr.sample(ring, sac_a.n_written, 16, sac_a.seed, sac_a._round - 1)
    for k in ("obs", "next_obs", "action", "reward", "discount", "mask"):
        assert _same_bits(batch[k], want[k]), k
    # resume: the learner's and the env's state_dict into the other pair; both continue with the same TimeSteps
    sac_b.load_state_dict(sac_a.state_dict())
    env_b.load_state_dict(env_a.state_dict())
    # (a ring restored without its contents offers nothing but its newest slot: the others are marked LAST)
    assert (np.delete(_snapshot(sac_b)["step_type"], (sac_b.n_written - 1) % C, axis=0) == L).all()
    sac_a.collect(3); sac_b.collect(3)
    ra, rb = _snapshot(sac_a), _snapshot(sac_b)
    new = [m % C for m in range(sac_a.n_written - 3, sac_a.n_written)]
    for k in ra:
        assert _same_bits(ra[k][new], rb[k][new]), k
    assert sac_b.n_written == sac_a.n_written == steps + 4 and not np.array_equal(ra["obs"], ring["obs"])
    assert all(torch.equal(x, y) for x, y in zip(sac_a.normalizer[1:], sac_b.normalizer[1:]))
    # evaluation: the mean action, squashed
    act = sac_a.act(ts.observation, deterministic=True)
    torch.cuda.synchronize()
    assert tuple(act.shape) == (E, sac_a.A) and act.dtype == torch.float64 and float(act.abs().max()) <= 1.0
    # the whole ring travels on request
    sd = sac_a.state_dict(include_replay=True)
    sac_b.load_state_dict(sd)
    assert _differing(_snapshot(sac_a), _snapshot(sac_b)) == []


# ---- it learns ---------------------------------------------------------------------------------------------------------
class _ToyEnv:
    """test_gpu_learn.py's toy task: the observation is 8 iid normals, the reward -mean((a - obs[:2] / 2)^2) of the
    observation the action answered; episodes of 5 steps end by termination and a FIRST follows.  The optimum is 0."""

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


TOY = dict(rounds=40, steps_per_round=8, grad_steps=16,
           sac=dict(hidden=(32, 32), capacity=32, batch_size=256, lr=1e-2, gamma=0.9, tau=0.05, init_alpha=0.1, seed=2))


def test_sac_learns_a_toy_task():
    """PPO's criterion unchanged: the mean reward of the last 5 of 40 rounds is at least half-way from that of the
    first 5 to the optimum 0."""
    torch.manual_seed(0)
    env = _ToyEnv(256, seed=1)
    sac = offpolicy.SAC(env, **TOY["sac"])
    log = sac.train(TOY["rounds"], TOY["steps_per_round"], TOY["grad_steps"])
    curve = [s["mean_reward"] for s in log]
    first5, last5 = float(np.mean(curve[:5])), float(np.mean(curve[-5:]))
    print(f"toy task: mean reward {first5:.4f} (first 5 rounds) -> {last5:.4f} (last 5); ratio {last5 / first5:.3f}; "
          f"alpha {log[-1]['alpha']:.4f}; curve {[round(c, 3) for c in curve[::5]]}")
    assert first5 < -0.1 and last5 >= 0.5 * first5
    assert all(np.isfinite(s["critic_loss"]) for s in log) and log[-1]["episodes"] > 0
