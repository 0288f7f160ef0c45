"""Host tests of the learner (include/learn/rp_learn.h, robopianist_amd/learning.py): the twin's GAE against a per-episode
textbook restatement, its Chan merge against numpy's moments, its MLP against torch, the binding's symbols, struct sizes
and argument validation (refused calls return before anything touches a device), `ppo_loss`, and one `update()` on a
rollout the twin made."""

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
from robopianist_amd import learning  # noqa: E402
from robopianist_amd.suite import specs  # noqa: E402

F, M, L = lr.FIRST, lr.MID, lr.LAST


# ---- the twin's GAE ------------------------------------------------------------------------------------------------------
def _textbook_gae(reward, discount, step_type, value, gamma, lam):
    """One env.  Split the slots into episodes -- an episode starts at a FIRST (or at slot 0) and ends at a LAST (or at
    slot T) -- then recurse inside each: A_t = delta_t + gamma lam d_{t+1} A_{t+1}, A past the episode's end = 0."""
    T = len(reward) - 1
    adv, valid = np.zeros(T), np.zeros(T, bool)
    starts = [0] + [t for t in range(1, T + 1) if step_type[t] == F]
    for i, s in enumerate(starts):
        end = starts[i + 1] - 1 if i + 1 < len(starts) else T    # the last slot of this episode
        lasts = [t for t in range(s, end + 1) if step_type[t] == L]
        if lasts:
            end = lasts[0]
        nxt = 0.0
        for t in range(end - 1, s - 1, -1):                      # the transitions t -> t + 1 inside the episode
            delta = reward[t + 1] + gamma * discount[t + 1] * value[t + 1] - value[t]
            adv[t] = nxt = delta + gamma * lam * discount[t + 1] * nxt
            valid[t] = True
    return adv, valid


def test_twin_gae_equals_the_textbook_per_episode():
    rng = np.random.default_rng(0)
    T = 12
    # termination (discount 0), truncation (discount 1), a forced FIRST with no LAST before it, a LAST at slot T and at 0
    seqs = [[F, M, M, L, F, M, L, F, M, M, M, M, M],
            [M, M, L, F, M, M, M, F, M, M, L, F, M],
            [L, F, M, M, M, M, M, M, M, M, M, M, L],
            [M] * 13,
            [M, L, F, L, F, L, F, M, M, M, M, L, F]]
    st = np.array(seqs, np.int32).T
    E = st.shape[1]
    reward = rng.normal(size=(T + 1, E)).astype(np.float32)
    value = rng.normal(size=(T + 1, E)).astype(np.float32)
    discount = np.ones((T + 1, E), np.float32)
    discount[3, 0] = 0.0; discount[10, 1] = 0.0          # the first LAST of env 0 and the second of env 1 terminate
    adv, ret, valid = lr.gae(reward, discount, st, value, 0.97, 0.9)
    for e in range(E):
        want, ok = _textbook_gae(reward[:, e].astype(np.float64), discount[:, e].astype(np.float64), st[:, e],
                                 value[:, e].astype(np.float64), 0.97, 0.9)
        assert valid[:, e].astype(bool).tolist() == ok.tolist(), e
        np.testing.assert_allclose(adv[:, e], want, rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(ret[:, e], want + value[:T, e], rtol=2e-6, atol=2e-7)
    assert valid[:, 3].all() and not valid[3, 0] and not valid[6, 0] and not valid[6, 1]
    # a NaN reward poisons its own episode only
    bad = reward.copy()
    bad[5, 0] = np.nan                                    # env 0, the episode of slots 4 .. 6
    adv2, _, valid2 = lr.gae(bad, discount, st, value, 0.97, 0.9)
    assert np.isnan(adv2[4, 0]) and np.array_equal(valid2, valid)
    keep = np.ones_like(adv, bool); keep[4:6, 0] = False
    assert np.array_equal(adv2[keep].view(np.uint32), adv[keep].view(np.uint32))


# ---- the twin's moments ----------------------------------------------------------------------------------------------------
def test_twin_chan_merge_equals_numpy_moments():
    rng = np.random.default_rng(1)
    parts = [(rng.normal(size=(n, 5)) * [1, 10, 0.1, 3, 1] + [0, 5, -2, 100, 0]).astype(np.float32) for n in (1, 7, 130)]
    count, mean, M2 = 0.0, np.zeros(5), np.zeros(5)
    for p in parts:
        count, mean, M2, mean32, inv32 = lr.moments(p, count, mean, M2, 1e-8)
    rows = np.concatenate(parts).astype(np.float64)
    assert count == len(rows)
    np.testing.assert_allclose(mean, rows.mean(0), rtol=1e-12)
    np.testing.assert_allclose(M2 / count, rows.var(0), rtol=1e-12)
    np.testing.assert_allclose(inv32, 1 / np.sqrt(rows.var(0) + 1e-8), rtol=1e-6)
    assert mean32.dtype == np.float32 and np.array_equal(mean32, mean.astype(np.float32))


# ---- the twin's networks ---------------------------------------------------------------------------------------------------
def _net(D, H1, H2, A, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(D, H1), torch.nn.Tanh(), torch.nn.Linear(H1, H2), torch.nn.Tanh(),
                                   torch.nn.Linear(H2, A))


def _weights(net):
    return [t.detach().numpy() for i in (0, 2, 4) for t in (net[i].weight, net[i].bias)]


def test_twin_mlp_equals_torch_float64():
    net = _net(37, 48, 32, 5, 0).double()
    x = np.random.default_rng(2).normal(size=(9, 37))
    want = net(torch.as_tensor(x)).detach().numpy()
    assert np.abs(lr.mlp(x, _weights(net)) - want).max() < 1e-12
    # the normaliser clips, each operation on its own
    xn = lr.normalize(np.array([[0.0, 50.0, -50.0]]), np.array([1.0, 0.0, 0.0]), np.array([2.0, 1.0, 1.0]), 5.0)
    assert xn.tolist() == [[-2.0, 5.0, -5.0]]


def test_twin_act_draws_the_planners_noise():
    net, crit = _net(4, 16, 16, 3, 1).double(), _net(4, 16, 16, 1, 2).double()
    obs = np.random.default_rng(3).normal(size=(6, 4)).astype(np.float32)
    ls = np.array([-0.5, 0.0, 0.3])
    kw = dict(mean=np.zeros(4), inv_std=np.ones(4), clip=10.0, actor=_weights(net), critic=_weights(crit), log_std=ls)
    a = lr.act(obs, seed=7, round_=2, **kw)
    z = lr.noise(7, 2, np.arange(6), 3).astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(a["action"], a["mu"] + np.exp(ls) * z, rtol=1e-15)
    want = torch.distributions.Normal(torch.as_tensor(a["mu"]), torch.as_tensor(np.exp(ls))).log_prob(
        torch.as_tensor(a["action"])).sum(-1).numpy()
    np.testing.assert_allclose(a["logp"], want, rtol=1e-9)
    part = lr.act(obs, seed=7, round_=2, row_first=2, row_count=3, **kw)
    # (the same rows and the same draws; the matrix products of another batch size may round in another order)
    assert np.abs(part["action"] - a["action"][2:5]).max() < 1e-14 and np.abs(part["value"] - a["value"][2:5]).max() < 1e-14
    det = lr.act(obs, deterministic=True, **kw)
    assert np.array_equal(det["action"], det["mu"]) and "logp" not in det
    assert (np.abs(a["env_action"]) <= 1).all()


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_dims_and_struct_sizes():
    L_ = learning.load_library()
    assert set(learning.EXPORTED_SYMBOLS) == {"rp_learn_pack", "rp_learn_act", "rp_learn_gae", "rp_learn_moments",
                                              "rp_learn_dim", "rp_learn_last_error"}
    assert [getattr(L_, s) for s in learning.EXPORTED_SYMBOLS]
    assert learning.dim("max_fields") == learning.MAX_FIELDS == 64
    assert learning.dim("max_hidden") == learning.MAX_HIDDEN == 256
    assert learning.dim("max_actions") == learning.MAX_ACTIONS == 128
    assert learning.dim("min_hidden") == learning.dim("hidden_multiple") == 16 and learning.dim("min_obs") == 1
    assert learning.dim("tile_rows") == 16 and learning.dim("moment_lanes") == 16
    assert learning.dim("nothing") == -1
    # the layouts of the header on the LP64 ABI
    assert ctypes.sizeof(learning.Field) == 16 and ctypes.sizeof(learning.Mlp) == 48
    assert ctypes.sizeof(learning.PackArgs) == 144 and ctypes.sizeof(learning.ActArgs) == 160
    assert ctypes.sizeof(learning.GaeArgs) == 104 and ctypes.sizeof(learning.MomentsArgs) == 88
    # and the library agrees: a zeroed block of the right size is refused for its contents, not for its size
    for entry in ("pack", "act", "gae", "moments"):
        a = learning.make_args(entry)
        assert learning.call_raw(entry, a) != 0 and "struct_size" not in learning.last_error()
        a.struct_size -= 8
        assert learning.call_raw(entry, a) != 0 and "struct_size" in learning.last_error()


_A = 0x1000   # a non-null address: a refused call never reads it


def _refused(entry, match, **values):
    args = learning.make_args(entry, **values)
    assert learning.call_raw(entry, args) != 0
    assert match in learning.last_error(), learning.last_error()


def test_argument_validation_refuses_before_any_launch():
    tab = learning.field_table([(_A, 3, learning.F32), (_A, 2, learning.F64)])
    pk = dict(fields=tab, n_fields=2, precision=64, step_type=_A, obs=_A, slot_reward=_A, slot_discount=_A,
              slot_step_type=_A, E=4, D=5, env_first=0, env_count=4)
    _refused("pack", "fields is NULL", **dict(pk, fields=None))
    _refused("pack", "n_fields", **dict(pk, n_fields=0))
    _refused("pack", "n_fields", **dict(pk, n_fields=65))
    _refused("pack", "precision", **dict(pk, precision=16))
    for name in ("step_type", "obs", "slot_reward", "slot_discount", "slot_step_type"):
        _refused("pack", "a pointer is NULL", **dict(pk, **{name: None}))
    _refused("pack", "together or not at all", **dict(pk, ep_return=_A))
    _refused("pack", "E must be", **dict(pk, E=0))
    _refused("pack", "D must be", **dict(pk, D=0))
    _refused("pack", "sum to 5", **dict(pk, D=6))
    _refused("pack", "outside the batch", **dict(pk, env_first=2, env_count=3))
    _refused("pack", "outside the batch", **dict(pk, env_first=-1))
    _refused("pack", "NULL pointer", **dict(pk, fields=learning.field_table([(None, 3, 0), (_A, 2, 0)])))
    _refused("pack", "width < 1", **dict(pk, fields=learning.field_table([(_A, 0, 0), (_A, 5, 0)])))
    _refused("pack", "dtype", **dict(pk, fields=learning.field_table([(_A, 3, 2), (_A, 2, 0)])))
    with pytest.raises(learning.LearnError):
        learning.field_table([])
    assert learning.call_raw("pack", learning.make_args("pack", **dict(pk, env_count=0))) == 0

    net = learning.Mlp(*([_A] * 6))
    ac = dict(obs=_A, mean=_A, inv_std=_A, obs_clip=5.0, actor=ctypes.pointer(net), critic=ctypes.pointer(net), log_std=_A,
              action=_A, logp=_A, env_action=_A, value=_A, precision=64, D=3, H1=16, H2=32, A=2, n_rows=4, row_first=0,
              row_count=4)
    for name in ("obs", "mean", "inv_std"):
        _refused("act", "a pointer is NULL", **dict(ac, **{name: None}))
    _refused("act", "obs_clip", **dict(ac, obs_clip=0.0))
    _refused("act", "neither", **dict(ac, actor=None, critic=None))
    _refused("act", "D must be", **dict(ac, D=0))
    for h in (0, 8, 24, 272):
        _refused("act", "H1 must be", **dict(ac, H1=h))
        _refused("act", "H2 must be", **dict(ac, H2=h))
    for A in (0, 129):
        _refused("act", "A must be", **dict(ac, A=A))
    _refused("act", "the actor has a NULL", **dict(ac, actor=ctypes.pointer(learning.Mlp(_A, _A, _A, None, _A, _A))))
    _refused("act", "the critic has a NULL", **dict(ac, critic=ctypes.pointer(learning.Mlp(None, _A, _A, _A, _A, _A))))
    _refused("act", "action and env_action", **dict(ac, env_action=None))
    _refused("act", "logp and log_std", **dict(ac, logp=None))
    _refused("act", "precision", **dict(ac, precision=0))
    _refused("act", "needs value", **dict(ac, value=None))
    _refused("act", "n_rows", **dict(ac, n_rows=0, row_count=0))
    _refused("act", "outside the batch", **dict(ac, row_first=3, row_count=2))
    assert learning.call_raw("act", learning.make_args("act", **dict(ac, row_count=0))) == 0
    assert learning.call_raw("act", learning.make_args("act", **dict(ac, actor=None, A=0, row_count=0))) == 0   # the critic alone

    ga = dict(reward=_A, discount=_A, step_type=_A, value=_A, adv=_A, ret=_A, valid=_A, gamma=0.99, T=3, E=4, env_count=4)
    for name in ("reward", "discount", "step_type", "value", "adv", "ret", "valid"):
        _refused("gae", "a pointer is NULL", **dict(ga, **{name: None}))
    _refused("gae", "T must be", **dict(ga, T=0))
    _refused("gae", "E must be", **dict(ga, E=0, env_count=0))
    _refused("gae", "outside the batch", **dict(ga, env_first=4, env_count=1))
    assert learning.call_raw("gae", learning.make_args("gae", **dict(ga, env_count=0))) == 0

    mo = dict(obs=_A, mean=_A, M2=_A, mean_f32=_A, inv_std_f32=_A, count=0.0, eps=1e-8, n_rows=5, D=3)
    for name in ("obs", "mean", "M2", "mean_f32", "inv_std_f32"):
        _refused("moments", "a pointer is NULL", **dict(mo, **{name: None}))
    _refused("moments", "D must be", **dict(mo, D=0))
    _refused("moments", "n_rows", **dict(mo, n_rows=0))
    _refused("moments", "count", **dict(mo, count=-1.0))
    _refused("moments", "count", **dict(mo, count=float("nan")))
    _refused("moments", "eps", **dict(mo, eps=0.0))
    with pytest.raises(TypeError):
        learning.make_args("gae", nothing=1)


# ---- the loss --------------------------------------------------------------------------------------------------------------
def _batch(n=64, A=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(n, A, generator=g, dtype=torch.float64)
    log_std = torch.tensor([-0.3, 0.0, 0.2], dtype=torch.float64)
    action = mu + log_std.exp() * torch.randn(n, A, generator=g, dtype=torch.float64)
    adv = torch.randn(n, generator=g, dtype=torch.float64)
    return mu, log_std, action, adv


def test_ppo_loss_surrogate_clip_and_gradient_signs():
    mu, log_std, action, adv = _batch()
    logp_old = learning.gaussian_logp(mu, log_std, action)
    want = torch.distributions.Normal(mu, log_std.exp()).log_prob(action).sum(-1)
    assert torch.allclose(logp_old, want, rtol=1e-12, atol=1e-12)
    value = ret = torch.zeros(len(adv), dtype=torch.float64)
    # at ratio 1 the surrogate is -mean(adv); the value loss and the entropy are what they say
    loss, s = learning.ppo_loss(mu, log_std, value + 1.0, action, logp_old, adv, ret, clip=0.2, vf_coef=0.5, ent_coef=0.01)
    assert abs(float(s["pg"]) + float(adv.mean())) < 1e-12 and abs(float(s["vf"]) - 0.5) < 1e-12
    ent = float(torch.distributions.Normal(mu[0], log_std.exp()).entropy().sum())
    assert abs(float(s["entropy"]) - ent) < 1e-12
    assert abs(float(loss) - (float(s["pg"]) + 0.25 - 0.01 * ent)) < 1e-12 and float(s["clip_fraction"]) == 0.0

    # one sample, the old log-probability shifted so that the ratio is r
    def one(r, a):
        m = mu[:1].clone().requires_grad_(True)
        ls = log_std.clone().requires_grad_(True)
        old = learning.gaussian_logp(m, ls, action[:1]).detach() - np.log(r)
        loss, s = learning.ppo_loss(m, ls, value[:1], action[:1], old, torch.tensor([a], dtype=torch.float64), ret[:1])
        loss.backward()
        return float(s["pg"]), m.grad, ls.grad, float(s["clip_fraction"])

    for a in (1.5, -1.5):
        pg, gm, gl, cf = one(1.1, a)                       # inside the band: the plain surrogate
        assert abs(pg + 1.1 * a) < 1e-12 and cf == 0.0 and float(gm.abs().max()) > 0
    pg, gm, gl, cf = one(1.5, 2.0)                         # above the band, positive advantage: clipped, no gradient
    assert abs(pg + 1.2 * 2.0) < 1e-12 and cf == 1.0 and float(gm.abs().max()) == 0 and float(gl.abs().max()) == 0
    pg, gm, gl, cf = one(0.5, -2.0)                        # below the band, negative advantage: clipped, no gradient
    assert abs(pg - 0.8 * 2.0) < 1e-12 and float(gm.abs().max()) == 0
    pg, gm, gl, cf = one(1.5, -2.0)                        # above the band, negative advantage: the min keeps it live
    assert abs(pg - 1.5 * 2.0) < 1e-12 and float(gm.abs().max()) > 0
    # descent moves the mean towards an action of positive advantage and away from one of negative advantage; log_std
    # grows for a positive advantage exactly where the action lies more than one sigma out
    for a in (1.0, -1.0):
        _, gm, gl, _ = one(1.0, a)
        towards = torch.sign(action[0] - mu[0])
        assert torch.equal(torch.sign(-gm[0]), towards * np.sign(a))
        far = ((action[0] - mu[0]).abs() > log_std.exp()).double() * 2 - 1
        assert torch.equal(torch.sign(-gl), far * np.sign(a))


# ---- one update on a rollout of the twin's -------------------------------------------------------------------------------------
class _SpecEnv:
    """As much of a batched Environment as PPO's constructor and update() read, on the CPU."""

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
        raise AssertionError("update() does not step the env")


def test_one_update_on_a_twin_made_rollout_changes_every_parameter():
    E, T, A = 6, 5, 3
    ppo = learning.PPO(_SpecEnv(E, (4, 3), A), hidden=(16, 32), horizon=T, epochs=2, minibatches=2, lr=1e-2, seed=5)
    assert (ppo.D, ppo.A, ppo.observation_keys) == (7, 3, ["o0", "o1"])
    rng = np.random.default_rng(4)
    st = np.full((T + 1, E), M, np.int32)
    st[0] = F; st[3, 1] = L; st[4, 1] = F; st[2, 4] = L; st[3, 4] = F
    obs = rng.normal(size=(T + 1, E, 7)).astype(np.float32)
    reward = rng.normal(size=(T + 1, E)).astype(np.float32)
    discount = np.ones((T + 1, E), np.float32)
    ls = ppo.log_std.detach().numpy().astype(np.float64)
    actor, critic = _weights(ppo.actor), _weights(ppo.critic)
    r = {"obs": obs, "reward": reward, "discount": discount, "step_type": st,
         "action": np.zeros((T, E, A), np.float32), "logp": np.zeros((T, E), np.float32),
         "value": np.zeros((T + 1, E), np.float32)}
    for t in range(T + 1):
        out = lr.act(obs[t], np.zeros(7), np.ones(7), ppo.obs_clip, actor if t < T else None, critic, ls, seed=5, round_=t)
        r["value"][t] = out["value"]
        if t < T:
            r["action"][t], r["logp"][t] = out["action"], out["logp"]
    r["adv"], r["ret"], r["valid"] = lr.gae(reward, discount, st, r["value"], ppo.gamma, ppo.lam)
    assert int(r["valid"].sum()) == T * E - 2
    before = [p.detach().clone() for p in ppo.optimizer.param_groups[0]["params"]]
    stats = ppo.update({k: torch.as_tensor(v) for k, v in r.items()})
    assert stats["batch"] == T * E - 2 and all(np.isfinite(v) for v in stats.values()), stats
    after = ppo.optimizer.param_groups[0]["params"]
    assert len(before) == 13
    for b, a in zip(before, after):
        assert bool((a != b).all()) and bool(torch.isfinite(a).all())
    # a snapshot is a snapshot: training on does not change one taken earlier (Adam's moments included)
    sd = ppo.state_dict()
    kept = [v["exp_avg"].clone() for v in sd["optimizer"]["state"].values()]
    ppo.update({k: torch.as_tensor(v) for k, v in r.items()})
    assert len(kept) == 13 and all(torch.equal(k, v["exp_avg"]) for k, v in zip(kept, sd["optimizer"]["state"].values()))
    assert not torch.equal(kept[0], ppo.optimizer.state_dict()["state"][0]["exp_avg"])
    # a PPO built again with the same seed starts from the same weights, whatever the global generator did meanwhile
    torch.manual_seed(123)
    again = learning.PPO(_SpecEnv(E, (4, 3), A), hidden=(16, 32), horizon=T, seed=5)
    assert all(torch.equal(x, y) for x, y in zip(before, again.optimizer.param_groups[0]["params"]))
    with pytest.raises(ValueError, match="multiples of 16"):
        learning.PPO(_SpecEnv(E, (4, 3), A), hidden=(20, 32))
    with pytest.raises(ValueError, match="step_canonical"):
        learning.PPO(object())


# ---- the checkpoint's layout and the initial parameters -------------------------------------------------------------------------
def test_state_dict_layout_and_initial_parameters_are_pinned():
    """Two instances of the same code agree whatever the code does; this compares with literals.  The digest was
    recorded by running these lines at the commit before the learners got their common base class."""
    E, D, A = 4, 7, 3
    ppo = learning.PPO(_SpecEnv(E, (4, 3), A), hidden=(16, 32), horizon=2, seed=5)
    sd = ppo.state_dict()
    f32, f64, i32, i64 = "torch.float32", "torch.float64", "torch.int32", "torch.int64"
    assert {k: lr.adam_tree(v) if k == "optimizer" else lr.state_tree(v) for k, v in sd.items()} == {
        "actor": lr.mlp_tree(D, A), "critic": lr.mlp_tree(D, 1), "log_std": (f32, (A,)),
        "optimizer": {"state": {}, "params": [list(range(13))]},
        "normalizer": {"count": "float", "mean": (f64, (D,)), "M2": (f64, (D,)), "mean_f32": (f32, (D,)),
                       "inv_std_f32": (f32, (D,))},
        "seed": "int", "round": "int", "started": "bool",
        "last": {"obs": (f32, (E, D)), "reward": (f32, (E,)), "discount": (f32, (E,)), "step_type": (i32, (E,)),
                 "value": (f32, (E,))},
        "episodes": {"ep_return": (f64, (E,)), "ep_len": (i32, (E,)), "done_return": (f64, (E,)), "done_len": (i64, (E,)),
                     "done_count": (i32, (E,))}}
    assert list(sd) == ["actor", "critic", "log_std", "optimizer", "normalizer", "seed", "round", "started", "last",
                        "episodes"]
    if torch.__version__ == "2.10.0+rocm7.0":   # (the initialisers' draws belong to torch)
        assert lr.digest(list(sd["actor"].values()) + list(sd["critic"].values()) + [sd["log_std"]]) == \
            "51a8854c8c0090ab0e528c5f76e4b64d00150c068d01856d281a2406ec59939b"
