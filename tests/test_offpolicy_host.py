"""Host tests of the off-policy learner (include/learn/rp_sac.h, robopianist_amd/offpolicy.py): the twin's sampler never
leaves the valid transitions and is uniform over them, its log-probability is the textbook change of variables, its
target the textbook TD target, the binding's symbols, struct sizes and argument validation (refused calls return before
anything touches a device), the torch losses' gradient signs, and one gradient step of `SAC` on a hand-made batch."""

from __future__ import annotations

import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import learn_reference as lr  # noqa: E402
import sac_reference as sr  # noqa: E402
from robopianist_amd import learning, offpolicy  # noqa: E402
from robopianist_amd.suite import specs  # noqa: E402

F, M, L = sr.FIRST, sr.MID, sr.LAST


# ---- the twin's sampler ------------------------------------------------------------------------------------------------
def _labelled_ring(C, E, n_written, step_type_of, D=3, A=2):
    """A ring whose rows say where they come from: obs = (TimeStep number, env, 0...), action = (number + 0.5, env)."""
    ring = {"obs": np.full((C, E, D), -1, np.float32), "action": np.full((C, E, A), -1, np.float32),
            "reward": np.zeros((C, E), np.float32), "discount": np.zeros((C, E), np.float32),
            "step_type": np.full((C, E), L, np.int32)}
    for m in range(max(0, n_written - C), n_written):
        s = m % C
        ring["obs"][s, :, 0], ring["obs"][s, :, 1] = m, np.arange(E)
        ring["action"][s, :, 0], ring["action"][s, :, 1] = m + 0.5, np.arange(E)
        ring["reward"][s], ring["discount"][s] = m + 0.25, m + 0.75
        ring["step_type"][s] = [step_type_of(m, e) for e in range(E)]
    return ring


@pytest.mark.parametrize("C, E, n_written", [(2, 1, 2), (4, 3, 3), (5, 7, 5), (5, 7, 13), (3, 2, 9), (6, 4, 1000)])
def test_twin_sampler_never_leaves_the_valid_transitions(C, E, n_written):
    rng = np.random.default_rng(C * 100 + n_written)
    types_ = rng.choice(np.array([F, M, M, M, L], np.int32), size=(n_written + 1, E))
    ring = _labelled_ring(C, E, n_written, lambda m, e: types_[m, e])
    B = 600
    out = sr.sample(ring, n_written, B, seed=5, round_=n_written)
    newest, Fc = (n_written - 1) % C, min(n_written, C)
    drawn = out["mask"] == 1
    assert np.array_equal(drawn, out["index"] >= 0) and np.array_equal(~drawn, out["tries"] == sr.TRIES + 1)
    for b in np.flatnonzero(drawn):
        m, e = int(out["obs"][b, 0]), int(out["obs"][b, 1])
        assert n_written - Fc <= m <= n_written - 2                      # never the newest TimeStep
        assert out["index"][b] == (m % C) * E + e and m % C != newest     # nor, from it, the oldest across the wrap
        assert out["next_obs"][b, 0] == m + 1 and out["next_obs"][b, 1] == e
        assert out["action"][b, 0] == m + 0.5 and out["action"][b, 1] == e
        assert out["reward"][b] == m + 1.25 and out["discount"][b] == m + 1.75
        assert types_[m, e] != L and types_[m + 1, e] != F
    for k in ("obs", "next_obs", "action", "reward", "discount"):
        assert (out[k][~drawn] == 0).all()
    assert (out["index"][~drawn] == -1).all()
    valid = sr.valid_transitions(ring["step_type"], n_written)
    assert valid.shape == (Fc - 1, E)
    if not valid.any():
        assert not drawn.any()
    # a row range leaves the other rows as they were
    part = sr.sample(ring, n_written, B, seed=5, round_=n_written, out={k: np.full_like(v, 9) for k, v in out.items()},
                     row_first=7, row_count=100)
    assert all(np.array_equal(part[k][7:107], out[k][7:107]) for k in out)
    assert all((part[k][:7] == 9).all() and (part[k][107:] == 9).all() for k in out if k != "tries")


def test_twin_sampler_is_uniform_over_the_valid_transitions():
    """n draws over V valid transitions: every count lies within 5 standard deviations of n / V (a binomial's)."""
    C, E, n_written = 5, 13, 12
    ring = _labelled_ring(C, E, n_written, lambda m, e: (F, M, M, M, M, L)[(m + e) % 6])
    valid = sr.valid_transitions(ring["step_type"], n_written)
    V = int(valid.sum())
    assert 0 < V < valid.size
    counts = np.zeros(C * E, np.int64)
    n = 0
    for round_ in range(4):
        out = sr.sample(ring, n_written, 50000, seed=(3 << 32) | 9, round_=round_)
        idx = out["index"][out["mask"] == 1]
        counts += np.bincount(idx, minlength=C * E)
        n += idx.size
    m = sr.candidates(n_written, C)
    want = np.zeros((C, E), bool)
    want[m % C] = valid
    assert (counts[~want.ravel()] == 0).all()
    p = 1.0 / V
    sigma = np.sqrt(n * p * (1 - p))
    assert np.abs(counts[want.ravel()] - n * p).max() < 5 * sigma, (counts[want.ravel()], n * p, sigma)
    # an invalid first attempt is retried: the share of masked rows is the invalid share to the power of the tries
    assert n >= 200000 * (1 - 2 * (1 - V / valid.size) ** sr.TRIES)


# ---- the twin's policy and target ----------------------------------------------------------------------------------------
def _net(n_in, H1, H2, n_out, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(n_in, H1), torch.nn.Tanh(), torch.nn.Linear(H1, H2), torch.nn.Tanh(),
                                   torch.nn.Linear(H2, n_out))


def _weights(net):
    return [t.detach().numpy() for i in (0, 2, 4) for t in (net[i].weight, net[i].bias)]


def test_twin_logp_is_the_textbook_change_of_variables():
    D, A, n = 6, 4, 40
    actor = _net(D, 16, 32, 2 * A, 0).double()
    with torch.no_grad():
        actor[4].bias[A:] += torch.tensor([0.0, 3.0, -7.0, -1.0])      # one log-std above the bounds, one below
    obs = np.random.default_rng(1).normal(size=(n, D)).astype(np.float32)
    out = sr.act(obs, np.zeros(D), np.ones(D), 10.0, _weights(actor), (-5.0, 2.0), seed=11, round_=4)
    assert (out["log_std"][:, 1] == 2.0).all() and (out["log_std"][:, 2] == -5.0).all()
    z = lr.noise(11, 4, np.arange(n), A).astype(np.float32).astype(np.float64)
    p = out["mu"] + np.exp(out["log_std"]) * z
    assert np.array_equal(p, out["pre"]) and np.array_equal(out["action"], np.tanh(p))
    normal = torch.distributions.Normal(torch.as_tensor(out["mu"]), torch.as_tensor(np.exp(out["log_std"])))
    keep = np.abs(p).max(1) < 6.0                                         # (1 - tanh^2 p itself cancels beyond)
    want = normal.log_prob(torch.as_tensor(p)).sum(-1).numpy() - np.log(1.0 - np.tanh(p) ** 2).sum(-1)
    assert keep.sum() > n // 2
    np.testing.assert_allclose(out["logp"][keep], want[keep], rtol=1e-9, atol=1e-9)
    # the well-conditioned form holds where the plain one has lost every digit
    big = np.array([[-40.0, -5.0, 0.0, 5.0, 40.0]])
    np.testing.assert_allclose(sr.log_one_minus_tanh2(big), [[-80 + 2 * sr.LN_2, np.log(1 - np.tanh(5.0) ** 2), 0.0,
                                                              np.log(1 - np.tanh(5.0) ** 2), -80 + 2 * sr.LN_2]],
                               rtol=1e-7, atol=1e-12)
    det = sr.act(obs, np.zeros(D), np.ones(D), 10.0, _weights(actor), deterministic=True)
    assert np.array_equal(det["pre"], det["mu"]) and "logp" not in det
    part = sr.act(obs, np.zeros(D), np.ones(D), 10.0, _weights(actor), seed=11, round_=4, row_first=3, row_count=5)
    assert np.abs(part["action"] - out["action"][3:8]).max() < 1e-14 and np.abs(part["logp"] - out["logp"][3:8]).max() < 1e-12


def test_twin_target_is_the_textbook_td_target():
    D, A, n = 5, 3, 30
    rng = np.random.default_rng(2)
    critics = [_net(D + A, 16, 16, 1, s).double() for s in (1, 2, 3)]
    mean, inv_std = rng.normal(size=D), 1 / rng.uniform(0.5, 2, D)
    nobs = (rng.normal(size=(n, D)) * 3).astype(np.float32)
    action = np.tanh(rng.normal(size=(n, A))).astype(np.float32)
    logp, reward = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    discount = np.where(rng.uniform(size=n) < 0.3, 0.0, 1.0).astype(np.float32)
    log_alpha = np.float32(-0.7)
    out = sr.target(nobs, action, logp, reward, discount, mean, inv_std, 2.0, 0.97, log_alpha, [_weights(c) for c in critics])
    xn = np.clip((nobs - mean) * inv_std, -2.0, 2.0)
    assert (np.abs(xn) == 2.0).any()
    xa = torch.as_tensor(np.concatenate([xn, action], 1))
    q = torch.stack([c(xa)[:, 0] for c in critics]).min(0).values.detach().numpy()
    np.testing.assert_allclose(out["q_min"], q, rtol=1e-12, atol=1e-13)
    want = reward + np.float64(np.float32(0.97)) * discount * (q - np.exp(np.float64(log_alpha)) * logp)
    np.testing.assert_allclose(out["y"], want, rtol=1e-12, atol=1e-13)
    assert np.array_equal(out["y"][discount == 0], reward[discount == 0].astype(np.float64))
    one = sr.target(nobs, action, logp, reward, discount, mean, inv_std, 2.0, 0.97, log_alpha, [_weights(critics[1])])
    assert (one["q_min"] >= out["q_min"]).all() and (one["q_min"] > out["q_min"]).any()


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_dims_and_struct_sizes():
    L_ = offpolicy.load_library()
    assert set(offpolicy.EXPORTED_SYMBOLS) == {"rp_sac_sample", "rp_sac_act", "rp_sac_target", "rp_sac_dim",
                                               "rp_sac_last_error"}
    assert [getattr(L_, s) for s in offpolicy.EXPORTED_SYMBOLS]
    assert offpolicy.dim("max_critics") == offpolicy.MAX_CRITICS == 4
    assert offpolicy.dim("sample_tries") == offpolicy.SAMPLE_TRIES == sr.TRIES == 4
    assert offpolicy.dim("tile_rows") == learning.dim("tile_rows") == 16
    assert offpolicy.dim("max_hidden") == learning.MAX_HIDDEN == 256
    assert offpolicy.dim("max_actions") == learning.MAX_ACTIONS == 128
    assert offpolicy.dim("nothing") == -1
    # the layouts of the header on the LP64 ABI
    assert ctypes.sizeof(offpolicy.SampleArgs) == 160 and ctypes.sizeof(offpolicy.ActArgs) == 144
    assert ctypes.sizeof(offpolicy.TargetArgs) == 152
    # and the library agrees: a zeroed block of the right size is refused for its contents, not for its size
    for entry in ("sample", "act", "target"):
        a = offpolicy.make_args(entry)
        assert offpolicy.call_raw(entry, a) != 0 and "struct_size" not in offpolicy.last_error()
        a.struct_size -= 8
        assert offpolicy.call_raw(entry, a) != 0 and "struct_size" in offpolicy.last_error()
    # the learner's library keeps its own symbols: the new kernels are not in it
    assert not hasattr(learning.load_library(), "rp_sac_sample")


_A = 0x1000   # a non-null address: a refused call never reads it


def _refused(entry, match, **values):
    args = offpolicy.make_args(entry, **values)
    assert offpolicy.call_raw(entry, args) != 0
    assert match in offpolicy.last_error(), offpolicy.last_error()


def test_argument_validation_refuses_before_any_launch():
    ptrs = ("ring_obs", "ring_action", "ring_reward", "ring_discount", "ring_step_type", "obs", "next_obs", "action",
            "reward", "discount", "mask")
    sa = dict({k: _A for k in ptrs}, index=_A, n_written=9, C=4, E=3, D=5, A=2, B=8, row_first=0, row_count=8)
    for name in ptrs:
        _refused("sample", "a pointer is NULL", **dict(sa, **{name: None}))
    _refused("sample", "C must be", **dict(sa, C=1))
    _refused("sample", "n_written", **dict(sa, n_written=1))
    for name in ("E", "D", "A"):
        _refused("sample", name + " must be", **dict(sa, **{name: 0}))
    _refused("sample", "B must be", **dict(sa, B=0, row_count=0))
    _refused("sample", "2^32", **dict(sa, E=2 ** 31 - 1))                   # (F - 1) E = 3 (2^31 - 1)
    _refused("sample", "outside the batch", **dict(sa, row_first=5, row_count=4))
    _refused("sample", "outside the batch", **dict(sa, row_first=-1))
    assert offpolicy.call_raw("sample", offpolicy.make_args("sample", **dict(sa, row_count=0))) == 0
    assert offpolicy.call_raw("sample", offpolicy.make_args("sample", **dict(sa, index=None, row_count=0))) == 0

    net = learning.Mlp(*([_A] * 6))
    ac = dict(obs=_A, mean=_A, inv_std=_A, obs_clip=5.0, log_std_min=-5.0, log_std_max=2.0, actor=ctypes.pointer(net),
              action=_A, logp=_A, env_action=_A, precision=64, D=3, H1=16, H2=32, A=2, n_rows=4, row_first=0, row_count=4)
    for name in ("obs", "mean", "inv_std", "action"):
        _refused("act", "a pointer is NULL", **dict(ac, **{name: None}))
    _refused("act", "actor is NULL", **dict(ac, actor=None))
    _refused("act", "obs_clip", **dict(ac, obs_clip=0.0))
    _refused("act", "log_std_min", **dict(ac, log_std_min=3.0))
    _refused("act", "D must be", **dict(ac, D=0))
    for h in (0, 8, 24, 272):
        _refused("act", "H1 must be", **dict(ac, H1=h))
        _refused("act", "H2 must be", **dict(ac, H2=h))
    for A in (0, 129):
        _refused("act", "A must be", **dict(ac, A=A))
    _refused("act", "the actor has a NULL", **dict(ac, actor=ctypes.pointer(learning.Mlp(_A, _A, _A, None, _A, _A))))
    _refused("act", "needs logp", **dict(ac, logp=None))
    _refused("act", "precision", **dict(ac, precision=0))
    _refused("act", "n_rows", **dict(ac, n_rows=0, row_count=0))
    _refused("act", "outside the batch", **dict(ac, row_first=3, row_count=2))
    assert offpolicy.call_raw("act", offpolicy.make_args("act", **dict(ac, row_count=0))) == 0
    assert offpolicy.call_raw("act", offpolicy.make_args("act", **dict(ac, logp=None, env_action=None, precision=0,
                                                                       deterministic=1, row_count=0))) == 0

    tab = offpolicy.critic_table([net, net])
    ta = dict(next_obs=_A, action=_A, logp=_A, reward=_A, discount=_A, mean=_A, inv_std=_A, obs_clip=5.0, gamma=0.99,
              log_alpha=_A, critics=tab, n_critics=2, y=_A, D=3, H1=16, H2=32, A=2, B=4, row_first=0, row_count=4)
    for name in ("next_obs", "action", "logp", "reward", "discount", "mean", "inv_std", "log_alpha", "y"):
        _refused("target", "a pointer is NULL", **dict(ta, **{name: None}))
    _refused("target", "critics is NULL", **dict(ta, critics=None))
    for n in (0, 5):
        _refused("target", "n_critics", **dict(ta, n_critics=n))
    _refused("target", "obs_clip", **dict(ta, obs_clip=-1.0))
    _refused("target", "D must be", **dict(ta, D=0))
    _refused("target", "H1 must be", **dict(ta, H1=8))
    _refused("target", "A must be", **dict(ta, A=129))
    _refused("target", "critic 1 has a NULL",
             **dict(ta, critics=offpolicy.critic_table([net, learning.Mlp(_A, _A, None, _A, _A, _A)])))
    _refused("target", "B must be", **dict(ta, B=0, row_count=0))
    _refused("target", "outside the batch", **dict(ta, row_first=1, row_count=4))
    assert offpolicy.call_raw("target", offpolicy.make_args("target", **dict(ta, row_count=0))) == 0
    with pytest.raises(offpolicy.LearnError):
        offpolicy.critic_table([])
    with pytest.raises(TypeError):
        offpolicy.make_args("target", nothing=1)


# ---- the losses --------------------------------------------------------------------------------------------------------------
def test_torch_epilogue_equals_the_twin_and_the_losses_have_the_right_gradient_signs():
    n, A = 6, 2
    g = torch.Generator().manual_seed(0)
    out = torch.randn(n, 2 * A, generator=g, dtype=torch.float64)
    out[0, A] = 5.0; out[1, A + 1] = -9.0                               # outside the bounds: clamped
    eps = torch.randn(n, A, generator=g, dtype=torch.float64)
    a, logp, p = offpolicy.squashed_gaussian(out, eps, (-5.0, 2.0))
    ls = np.clip(out[:, A:].numpy(), -5.0, 2.0)
    want = ((-0.5 * eps.numpy() ** 2 - ls) - sr.log_one_minus_tanh2(p.numpy())).sum(1) - 0.5 * A * sr.LN_2PI
    np.testing.assert_allclose(logp.numpy(), want, rtol=1e-12)
    assert torch.equal(a, torch.tanh(p))
    mask = torch.tensor([1, 1, 0, 1, 0, 1], dtype=torch.float64)
    # the critics: descent moves Q towards y on the rows of mask 1 and leaves the others alone
    y = torch.tensor([1.0, -1.0, 5.0, 0.5, -5.0, 0.0], dtype=torch.float64)
    q = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    loss = offpolicy.critic_loss([q, q + 0.0], y, mask)
    assert abs(float(loss.detach()) - 2 * 0.5 * float((y ** 2 * mask).sum() / 4)) < 1e-12
    loss.backward()
    assert torch.equal(torch.sign(-q.grad), torch.sign(y) * mask)
    # the actor: descent raises Q(a_new) and, alpha > 0, lowers logp; masked rows carry no gradient
    log_alpha = torch.tensor([-0.5], dtype=torch.float64, requires_grad=True)
    lp, qn = logp.detach().clone().requires_grad_(True), torch.zeros(n, dtype=torch.float64, requires_grad=True)
    offpolicy.actor_loss(log_alpha, lp, qn, mask).backward()
    assert (qn.grad[mask == 1] < 0).all() and (lp.grad[mask == 1] > 0).all()
    assert (qn.grad[mask == 0] == 0).all() and (lp.grad[mask == 0] == 0).all() and log_alpha.grad is None
    assert torch.allclose(lp.grad[mask == 1], torch.full((4,), float(np.exp(-0.5)) / 4, dtype=torch.float64))
    # the temperature: descent raises alpha while the entropy (-logp) is below its target and lowers it above
    for shift, sign in ((+3.0, +1.0), (-3.0, -1.0)):
        la = torch.tensor([0.0], dtype=torch.float64, requires_grad=True)
        lp2 = torch.full((n,), shift, dtype=torch.float64, requires_grad=True)    # entropy -shift, target -(-1) ...
        offpolicy.alpha_loss(la, lp2, 1.0, mask).backward()
        assert lp2.grad is None and float(torch.sign(-la.grad)) == sign
    # the gradient reaches the head through tanh and through the clamp only inside the bounds
    o = out.clone().requires_grad_(True)
    a2, lp3, _ = offpolicy.squashed_gaussian(o, eps, (-5.0, 2.0))
    (lp3.sum() + a2.sum()).backward()
    assert o.grad[0, A] == 0 and o.grad[1, A + 1] == 0 and (o.grad[2:] != 0).all()


# ---- one gradient step on a hand-made batch ------------------------------------------------------------------------------
class _SpecEnv:
    """As much of a batched Environment as SAC's constructor and gradient_step() read, on the CPU."""

    def __init__(self, E, widths, A):
        self.n_envs = E
        self.physics = types.SimpleNamespace(device=torch.device("cpu"), dtype=torch.float64)
        self._ospec = {f"o{i}": specs.Array((w,), np.float64) for i, w in enumerate(widths)}
        self._aspec = specs.BoundedArray((A,), np.float64, -2.0, 3.0)

    def observation_spec(self):
        return self._ospec

    def action_spec(self):
        return self._aspec

    def step_canonical(self, action, bounds, clip=False):
        raise AssertionError("gradient_step() does not step the env")


def test_one_gradient_step_changes_every_parameter_and_moves_the_targets_by_tau():
    E, A, B = 4, 3, 32
    sac = offpolicy.SAC(_SpecEnv(E, (4, 3), A), hidden=(16, 32), n_critics=3, capacity=4, batch_size=B, lr=1e-2, tau=0.25,
                        seed=5)
    assert (sac.D, sac.A, sac.observation_keys, sac.target_entropy) == (7, 3, ["o0", "o1"], -3.0)
    assert tuple(sac.actor[4].weight.shape) == (2 * A, 32) and tuple(sac.critics[0][0].weight.shape) == (16, 7 + A)
    assert all(torch.equal(p, q) for c, t in zip(sac.critics, sac.targets) for p, q in zip(c.parameters(), t.parameters()))
    rng = np.random.default_rng(6)
    batch = {"obs": torch.as_tensor(rng.normal(size=(B, 7)).astype(np.float32)),
             "action": torch.as_tensor(np.tanh(rng.normal(size=(B, A))).astype(np.float32)),
             "y": torch.as_tensor(rng.normal(size=B).astype(np.float32)),
             "mask": torch.as_tensor((rng.uniform(size=B) < 0.9).astype(np.float32))}
    params = list(sac.actor.parameters()) + [p for c in sac.critics for p in c.parameters()] + [sac.log_alpha]
    before = [p.detach().clone() for p in params]
    t_before = [p.detach().clone() for t in sac.targets for p in t.parameters()]
    stats = sac.gradient_step(batch)
    assert all(bool(torch.isfinite(v).all()) for v in stats.values()), stats
    assert len(before) == 6 + 18 + 1
    for b, a in zip(before, params):
        assert bool((a != b).all()) and bool(torch.isfinite(a).all())
    src = [p.detach() for c in sac.critics for p in c.parameters()]
    for tb, ta, s in zip(t_before, [p for t in sac.targets for p in t.parameters()], src):
        assert torch.allclose(ta, tb + 0.25 * (s - tb), rtol=1e-6, atol=1e-7) and not torch.equal(ta, tb)
    # a snapshot is a snapshot, and it restores every part
    sd = sac.state_dict(include_replay=True)
    kept = sd["actor"]["0.weight"].clone()
    sac.gradient_step(batch)
    assert torch.equal(kept, sd["actor"]["0.weight"]) and not torch.equal(kept, sac.actor[0].weight)
    again = offpolicy.SAC(_SpecEnv(E, (4, 3), A), hidden=(16, 32), n_critics=3, capacity=4, batch_size=B, lr=1e-2,
                          tau=0.25, seed=77)
    again.load_state_dict(sd)
    assert torch.equal(again.actor[0].weight, kept) and again.seed == 5 and float(again.log_alpha.detach()) == float(sd["log_alpha"])
    s1, s2 = again.gradient_step(batch), None
    sac.load_state_dict(sd)
    s2 = sac.gradient_step(batch)
    assert all(torch.equal(s1[k], s2[k]) for k in s1)                      # (the generator's state travels too)
    # a SAC built again with the same seed starts from the same weights, whatever the global generator did meanwhile
    torch.manual_seed(123)
    fresh = offpolicy.SAC(_SpecEnv(E, (4, 3), A), hidden=(16, 32), n_critics=3, capacity=4, batch_size=B, seed=5)
    other = offpolicy.SAC(_SpecEnv(E, (4, 3), A), hidden=(16, 32), n_critics=3, capacity=4, batch_size=B, seed=5)
    assert all(torch.equal(x, y) for x, y in zip(fresh.actor.parameters(), other.actor.parameters()))
    with pytest.raises(ValueError, match="multiples of 16"):
        offpolicy.SAC(_SpecEnv(E, (4, 3), A), hidden=(20, 32))
    with pytest.raises(ValueError, match="capacity"):
        offpolicy.SAC(_SpecEnv(E, (4, 3), A), capacity=1)
    with pytest.raises(ValueError, match="n_critics"):
        offpolicy.SAC(_SpecEnv(E, (4, 3), A), n_critics=5)
    with pytest.raises(ValueError, match="step_canonical"):
        offpolicy.SAC(object())
    with pytest.raises(offpolicy.LearnError, match="collect"):
        fresh.update()


# ---- the checkpoint's layout and the initial parameters -------------------------------------------------------------------------
def test_state_dict_layout_and_initial_parameters_are_pinned():
    """Two instances of the same code agree whatever the code does; this compares with literals.  The digest was
    recorded by running these lines at the commit before the learners got their common base class."""
    E, D, A, C = 4, 7, 3, 4
    sac = offpolicy.SAC(_SpecEnv(E, (4, 3), A), hidden=(16, 32), n_critics=3, capacity=C, batch_size=8, seed=5)
    f32, f64, i32, i64 = "torch.float32", "torch.float64", "torch.int32", "torch.int64"
    expected = {
        "actor": lr.mlp_tree(D, 2 * A), "critics": [lr.mlp_tree(D + A, 1)] * 3, "targets": [lr.mlp_tree(D + A, 1)] * 3,
        "log_alpha": (f32, (1,)),
        "optimizers": {"actor": {"state": {}, "params": [list(range(6))]},
                       "critic": {"state": {}, "params": [list(range(18))]},
                       "alpha": {"state": {}, "params": [[0]]}},
        "normalizer": {"count": "float", "mean": (f64, (D,)), "M2": (f64, (D,)), "mean_f32": (f32, (D,)),
                       "inv_std_f32": (f32, (D,))},
        "seed": "int", "round": "int", "n_written": "int", "generator": ("torch.uint8", (5056,)),
        "newest": {"obs": (f32, (E, D)), "reward": (f32, (E,)), "discount": (f32, (E,)), "step_type": (i32, (E,))},
        "episodes": {"ep_return": (f64, (E,)), "ep_len": (i32, (E,)), "done_return": (f64, (E,)), "done_len": (i64, (E,)),
                     "done_count": (i32, (E,))}}
    replay = {"obs": (f32, (C, E, D)), "reward": (f32, (C, E)), "discount": (f32, (C, E)), "step_type": (i32, (C, E)),
              "action": (f32, (C, E, A))}
    for include_replay in (False, True):
        sd = sac.state_dict(include_replay=include_replay)
        want = dict(expected, replay=replay) if include_replay else expected
        assert {k: {n: lr.adam_tree(o) for n, o in v.items()} if k == "optimizers" else lr.state_tree(v)
                for k, v in sd.items()} == want
        assert list(sd) == list(want)
    if torch.__version__ == "2.10.0+rocm7.0":   # (the initialisers' draws belong to torch)
        params = [sd["actor"]] + sd["critics"] + sd["targets"]
        assert lr.digest([v for m in params for v in m.values()] + [sd["log_alpha"]]) == \
            "4171ee497d8533ae8ed74d6524f952a590fbcc1f1ce401fde65a762ac6694d1d"
