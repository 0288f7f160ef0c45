"""Host tests of DroQ (include/learn/rp_droq.h, robopianist_amd/droq.py): the twin is torch's Linear -> dropout ->
LayerNorm -> ReLU critic with the twin's own masks, the mask rule (its rate, its independence between critics, layers
and rounds, and of the row range), the conditioning of the cases the GPU tests run, the binding's symbols, struct sizes
and argument validation (refused calls return before anything touches a device), and the class on a hand-made batch.

Conditioning.  The GPU tests hold the kernel to 8 times the error of a float32 restatement; that is only fair where a
float32 restatement in another summation order lies close to the first one.  Here a second restatement with the k order
of every product and the unit order of every LayerNorm sum shuffled must lie within 4 times the first one's error, for
every case, with and without dropout, for 1 .. 4 critics and for y, q_min and every critic's own value.  The seeds of
droq_cases.SEEDS were chosen for that on the CPU (the ratios of the candidates are recorded there).
"""

from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import droq_cases as dc  # noqa: E402
import droq_reference as dr  # noqa: E402
from test_offpolicy_host import _SpecEnv  # noqa: E402
from robopianist_amd import droq, learning, offpolicy  # noqa: E402


EPS = float(np.float32(dc.LN_EPS))   # ln_eps is a float of the argument block: torch is given the value the kernel gets


# ---- the twin ------------------------------------------------------------------------------------------------------------
def _inputs(rows, D, A, seed):
    rng = np.random.default_rng(seed)
    return dict(next_obs=(rng.normal(size=(rows, D)) * 3).astype(np.float32),
                action=np.tanh(rng.normal(size=(rows, A))).astype(np.float32), logp=rng.normal(size=rows).astype(np.float32),
                reward=rng.normal(size=rows).astype(np.float32),
                discount=np.where(rng.uniform(size=rows) < 0.3, 0.0, 1.0).astype(np.float32), mean=rng.normal(size=D),
                inv_std=1 / rng.uniform(0.5, 2, D), clip=2.0, gamma=0.97, log_alpha=np.float32(-0.7))


def test_twin_is_torch_with_explicit_masks_and_the_textbook_td_target():
    rows, D, H1, H2, A, p = 30, 5, 48, 16, 3, 0.5
    kw = _inputs(rows, D, A, 2)
    nets = [dc.critic_net(D + A, H1, H2, p, s).double() for s in (1, 2, 3)]
    scale = 1.0 / (1.0 - p)
    out = dr.target(critics=[dc.host(c) for c in nets], threshold=dr.drop_threshold(p), keep_scale=scale, ln_eps=dc.LN_EPS,
                    seed=dc.SEED, round_=4, **kw)
    xn = np.clip((kw["next_obs"] - kw["mean"]) * kw["inv_std"], -2.0, 2.0)
    assert (np.abs(xn) == 2.0).any()
    x = torch.as_tensor(np.concatenate([xn, kw["action"]], 1))
    qs = []
    for i, net in enumerate(nets):
        h = x
        for L, (lin, ln) in enumerate(((0, 2), (4, 6))):
            keep = dr.masks(np.arange(rows), net[lin].out_features, i, L, dc.SEED, 4, dr.drop_threshold(p))
            assert 0 < keep.sum() < keep.size
            assert np.array_equal(keep, out["masks"][i][L])
            h = net[lin](h) * torch.as_tensor(keep.astype(np.float64)) * np.float64(np.float32(scale))
            h = torch.relu(F.layer_norm(h, (h.shape[1],), net[ln].weight, net[ln].bias, EPS))
        qs.append(net[8](h)[:, 0].detach().numpy())
    np.testing.assert_allclose(out["q"], np.stack(qs), rtol=1e-12, atol=1e-13)
    q = np.stack(qs).min(0)
    np.testing.assert_allclose(out["q_min"], q, rtol=1e-12, atol=1e-13)
    want = kw["reward"] + np.float64(np.float32(0.97)) * kw["discount"] * (q - np.exp(np.float64(kw["log_alpha"])) * kw["logp"])
    np.testing.assert_allclose(out["y"], want, rtol=1e-12, atol=1e-13)
    stop = kw["discount"] == 0
    assert stop.any() and np.array_equal(out["y"][stop], kw["reward"][stop].astype(np.float64))


def test_twin_without_dropout_is_the_modules_in_eval_mode():
    rows, D, H1, H2, A = 20, 6, 32, 64, 4
    kw = _inputs(rows, D, A, 3)
    nets = [dc.critic_net(D + A, H1, H2, 0.3, s, eps=EPS).double().eval() for s in (4, 5)]
    out = dr.target(critics=[dc.host(c) for c in nets], threshold=0, keep_scale=1.0, ln_eps=dc.LN_EPS, seed=1, round_=2, **kw)
    assert all(m.all() for pair in out["masks"] for m in pair)
    xn = np.clip((kw["next_obs"] - kw["mean"]) * kw["inv_std"], -2.0, 2.0)
    x = torch.as_tensor(np.concatenate([xn, kw["action"]], 1))
    with torch.no_grad():
        q = torch.stack([c(x)[:, 0] for c in nets]).numpy()
    np.testing.assert_allclose(out["q"], q, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(out["q_min"], q.min(0), rtol=1e-12, atol=1e-13)


# ---- the mask rule -------------------------------------------------------------------------------------------------------
def test_mask_rule():
    rows, H = np.arange(256), 256                                        # 2^16 units
    for p in (0.01, 0.5):
        keep = dr.masks(rows, H, 0, 0, dc.SEED, 1, dr.drop_threshold(p))
        n = keep.size
        sigma = np.sqrt(n * p * (1 - p))
        assert n == 2 ** 16 and abs(keep.sum() - n * (1 - p)) < 4 * sigma, (p, keep.sum(), n * (1 - p), sigma)
    assert dr.masks(rows, H, 0, 0, dc.SEED, 1, dr.drop_threshold(0.0)).all()
    assert dr.drop_threshold(0.0) == droq.drop_threshold(0.0) == 0
    assert dr.drop_threshold(0.5) == droq.drop_threshold(0.5) == 2 ** 31
    assert droq.drop_threshold(1.0) == 2 ** 32 - 1 and droq.drop_threshold(0.01) == int(0.01 * 2 ** 32)
    t = dr.drop_threshold(0.5)
    base = dr.masks(rows, H, 0, 0, dc.SEED, 1, t)
    for other in (dr.masks(rows, H, 1, 0, dc.SEED, 1, t), dr.masks(rows, H, 0, 1, dc.SEED, 1, t),
                  dr.masks(rows, H, 0, 0, dc.SEED, 2, t), dr.masks(rows, H, 0, 0, dc.SEED + 1, 1, t)):
        assert 0.4 < (other != base).mean() < 0.6
    # critic 0's second layer is not critic 1's first: the counter word is 32 + 2 i + L
    assert not np.array_equal(dr.masks(rows, H, 0, 1, dc.SEED, 1, t), dr.masks(rows, H, 1, 0, dc.SEED, 1, t)[:, ::-1])
    # a row's mask does not depend on the range it is asked in, nor on the width of a narrower layer's other units
    assert np.array_equal(dr.masks(np.arange(7, 19), H, 2, 1, dc.SEED, 1, t), dr.masks(rows, H, 2, 1, dc.SEED, 1, t)[7:19])
    assert np.array_equal(dr.masks(rows, 48, 2, 1, dc.SEED, 1, t), dr.masks(rows, H, 2, 1, dc.SEED, 1, t)[:, :48])
    kw = _inputs(40, 5, 3, 7)
    nets = [dc.host(dc.critic_net(8, 16, 32, 0.5, s)) for s in (1, 2)]
    a = dict(critics=nets, threshold=t, keep_scale=2.0, seed=3, round_=9, **kw)
    full, part = dr.target(**a), dr.target(row_first=11, row_count=13, **a)
    assert np.abs(part["y"] - full["y"][11:24]).max() < 1e-12 and np.abs(part["q"] - full["q"][:, 11:24]).max() < 1e-12
    assert all(np.array_equal(pm, fm[11:24]) for pp, fp in zip(part["masks"], full["masks"]) for pm, fm in zip(pp, fp))


def test_the_sums_of_the_twin_follow_the_header():
    """Every unit belongs to one lane, a lane's units ascend, and the tree is the balanced one over the lanes in order."""
    for H in range(16, 257, 16):
        units = dr.lane_units(H)
        assert sorted(n for u in units for n in u) == list(range(H)) and all(u == sorted(u) for u in units)
        assert all(u[:4] == [4 * j, 4 * j + 1, 4 * j + 2, 4 * j + 3] for j, u in enumerate(units) if u)
    x = np.random.default_rng(0).normal(size=(3, 48)).astype(np.float32)
    p = [np.float32(0)] * 16
    for j, units in enumerate(dr.lane_units(48)):
        for n in units:
            p[j] = p[j] + x[1, n]
    while len(p) > 1:
        p = [p[i] + p[i + 1] for i in range(0, len(p), 2)]
    assert dr.row_sum(x)[1] == p[0] and dr.row_sum(x).dtype == np.float32


# ---- the conditioning of the GPU cases -----------------------------------------------------------------------------------
def test_the_wide_cases_are_what_the_first_four_are_not():
    tile = droq.dim("tile_rows")
    assert all(c[0] % tile and (c[1] + c[4]) % 16 and c[2] >= c[3] for c in dc.CASES)
    assert dc.ALL_CASES == dc.CASES + dc.WIDE_CASES and len(set(dc.ALL_CASES)) == 8 and set(dc.SEEDS) == set(dc.ALL_CASES)
    a, b, c, d = dc.WIDE_CASES
    assert all(w[0] % tile == 0 for w in dc.WIDE_CASES)                  # only full tiles: no invalid row in the last one
    assert a[2] < a[3] and a[0] == 2 * tile                              # H1 < H2
    assert b[0] == tile and b[1] + b[4] == 16                            # one full tile; D + A = 16
    assert (c[2], c[3]) == (16, learning.MAX_HIDDEN) and (c[1] + c[4]) % 32 == 0   # narrowest into widest; exact k stages
    assert (d[2], d[3]) == (learning.MAX_HIDDEN, 16) and d[0] == 3 * tile           # widest into narrowest


@pytest.mark.parametrize("case", dc.ALL_CASES, ids=dc.case_id)
def test_gpu_cases_are_well_conditioned(case):
    p = dc.problem(case)
    assert case[0] >= 5
    worst = 0.0
    for mode_n, err in p.err32.items():
        assert set(err) == set(dc.keys(mode_n[1]))
        for k, e in err.items():
            assert e > 0, (mode_n, k)
            ratio = p.err_perm[mode_n][k] / e
            worst = max(worst, ratio)
            assert ratio <= 4, (case, mode_n, k, p.err_perm[mode_n][k], e)
    print(f"conditioning {case}: the permuted restatement's error is at most {worst:.2f} x the first one's")
    stop = p.kw["discount"] == 0
    assert stop.any() and (p.ref["on", 2]["y"][stop] == p.kw["reward"][stop]).all()
    assert not np.array_equal(p.ref["on", 1]["q0"], p.ref["off", 1]["q0"])          # the dropout of the case drops something


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_dims_and_struct_sizes():
    L_ = droq.load_library()
    assert set(droq.EXPORTED_SYMBOLS) == {"rp_droq_target", "rp_droq_dim", "rp_droq_last_error"}
    assert [getattr(L_, s) for s in droq.EXPORTED_SYMBOLS]
    assert droq.dim("max_critics") == droq.MAX_CRITICS == offpolicy.MAX_CRITICS == 4
    assert droq.dim("tile_rows") == offpolicy.dim("tile_rows") == 16
    assert droq.dim("max_hidden") == learning.MAX_HIDDEN == 256
    assert droq.dim("max_actions") == learning.MAX_ACTIONS == 128
    assert droq.dim("nothing") == -1 and droq.dim("sample_tries") == -1
    assert droq.COUNTER == dr.COUNTER == 32
    # the layouts of the header on the LP64 ABI
    assert ctypes.sizeof(droq.Critic) == 80 and ctypes.sizeof(droq.TargetArgs) == 184
    a = droq.make_args("target")
    assert droq.call_raw("target", a) != 0 and "struct_size" not in droq.last_error()
    a.struct_size -= 8
    assert droq.call_raw("target", a) != 0 and "struct_size" in droq.last_error()
    # each library keeps its own symbols
    assert not hasattr(offpolicy.load_library(), "rp_droq_target") and not hasattr(L_, "rp_sac_target")


_A = 0x1000   # a non-null address: a refused call never reads it


def _refused(match, **values):
    args = droq.make_args("target", **values)
    assert droq.call_raw("target", args) != 0
    assert match in droq.last_error(), droq.last_error()


def test_argument_validation_refuses_before_any_launch():
    c = droq.Critic(learning.Mlp(*([_A] * 6)), _A, _A, _A, _A)
    tab = droq.critic_table([c, c])
    ta = dict(next_obs=_A, action=_A, logp=_A, reward=_A, discount=_A, mean=_A, inv_std=_A, obs_clip=5.0, gamma=0.99,
              log_alpha=_A, critics=tab, n_critics=2, y=_A, q_min=_A, q=_A, drop_threshold=7, keep_scale=1.0, ln_eps=1e-5,
              D=3, H1=16, H2=32, A=2, B=4, row_first=0, row_count=4)
    for name in ("next_obs", "action", "logp", "reward", "discount", "mean", "inv_std", "log_alpha", "y"):
        _refused("a pointer is NULL", **dict(ta, **{name: None}))
    _refused("critics is NULL", **dict(ta, critics=None))
    for n in (0, 5):
        _refused("n_critics", **dict(ta, n_critics=n))
    _refused("obs_clip", **dict(ta, obs_clip=-1.0))
    for bad in (0.0, -1.0, float("nan")):
        _refused("keep_scale must be > 0", **dict(ta, keep_scale=bad))
        _refused("ln_eps must be > 0", **dict(ta, ln_eps=bad))
    _refused("D must be", **dict(ta, D=0))
    for h in (0, 8, 24, 272):
        _refused("H1 must be", **dict(ta, H1=h))
        _refused("H2 must be", **dict(ta, H2=h))
    for A in (0, 129):
        _refused("A must be", **dict(ta, A=A))
    _refused("critic 1 has a NULL",
             **dict(ta, critics=droq.critic_table([c, droq.Critic(learning.Mlp(_A, _A, None, _A, _A, _A), _A, _A, _A, _A)])))
    for k in range(4):
        ln = [_A] * 4
        ln[k] = None
        _refused("the LayerNorm of critic 1 has a NULL",
                 **dict(ta, critics=droq.critic_table([c, droq.Critic(learning.Mlp(*([_A] * 6)), *ln)])))
    _refused("B must be", **dict(ta, B=0, row_count=0))
    _refused("outside the batch", **dict(ta, row_first=1, row_count=4))
    _refused("outside the batch", **dict(ta, row_first=-1))
    assert droq.last_error().startswith("rp_droq_target: ")
    assert droq.call_raw("target", droq.make_args("target", **dict(ta, row_count=0))) == 0
    assert droq.call_raw("target", droq.make_args("target", **dict(ta, q=None, q_min=None, drop_threshold=0, row_count=0))) == 0
    with pytest.raises(droq.LearnError):
        droq.critic_table([])
    with pytest.raises(droq.LearnError):
        droq.critic_table([c] * 5)
    with pytest.raises(TypeError):
        droq.make_args("target", nothing=1)


# ---- the class on a hand-made batch ----------------------------------------------------------------------------------------
def _droq(seed=5, **kw):
    E, A = 4, 3
    args = dict(hidden=(16, 32), n_critics=3, capacity=4, batch_size=32, lr=1e-2, tau=0.25, seed=seed, dropout=0.25, utd=3)
    args.update(kw)
    return droq.DroQ(_SpecEnv(E, (4, 3), A), **args)


def test_constructor_and_module_layout():
    from torch import nn
    d = _droq()
    assert (d.D, d.A, d.dropout, d.utd, d.ln_eps) == (7, 3, 0.25, 3, 1e-5) and isinstance(d, offpolicy.SAC)
    kinds = [nn.Linear, nn.Dropout, nn.LayerNorm, nn.ReLU, nn.Linear, nn.Dropout, nn.LayerNorm, nn.ReLU, nn.Linear]
    for net in d.critics + d.targets:
        assert [type(m) for m in net] == kinds and net.training
        assert tuple(net[0].weight.shape) == (16, 10) and tuple(net[4].weight.shape) == (32, 16)
        assert tuple(net[8].weight.shape) == (1, 32) and net[1].p == net[5].p == 0.25
        assert net[2].normalized_shape == (16,) and net[6].normalized_shape == (32,) and net[2].eps == net[6].eps == 1e-5
    assert [type(m) for m in d.actor] == [nn.Linear, nn.Tanh, nn.Linear, nn.Tanh, nn.Linear]
    assert tuple(d.actor[4].weight.shape) == (6, 32)
    assert all(torch.equal(p, q) for c, t in zip(d.critics, d.targets) for p, q in zip(c.parameters(), t.parameters()))
    assert all(not p.requires_grad for t in d.targets for p in t.parameters())
    # the minibatch buffers hold utd ranges; minibatch() is a view of the last one
    assert tuple(d._u_obs.shape) == (96, 7) and tuple(d.minibatch()["obs"].shape) == (32, 7)
    assert d.minibatch()["y"].data_ptr() == d._u_y[64:].data_ptr()
    # the same seed gives the same weights whatever the global generator did meanwhile, and the actor is SAC's
    torch.manual_seed(123)
    again, sac = _droq(), offpolicy.SAC(_SpecEnv(4, (4, 3), 3), hidden=(16, 32), n_critics=3, capacity=4, batch_size=32, seed=5)
    assert all(torch.equal(x, y) for x, y in zip(d.critics[2].parameters(), again.critics[2].parameters()))
    assert all(torch.equal(x, y) for x, y in zip(d.actor.parameters(), sac.actor.parameters()))
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="dropout"):
            _droq(dropout=bad)
    with pytest.raises(ValueError, match="utd"):
        _droq(utd=0)
    with pytest.raises(ValueError, match="ln_eps"):
        _droq(ln_eps=0.0)
    with pytest.raises(ValueError, match="multiples of 16"):
        _droq(hidden=(20, 32))
    with pytest.raises(ValueError, match="n_critics"):
        _droq(n_critics=5)
    with pytest.raises(droq.LearnError, match="collect"):
        d.update()
    assert _droq(dropout=0.0)._threshold == 0 and _droq(dropout=0.0)._keep_scale == 1.0


def test_critic_table_reads_the_parameters_in_place_and_refuses_a_non_contiguous_one():
    d = _droq()
    net = d.targets[1]
    c = d._critic_table(net)
    assert [c.net.w1, c.net.b1, c.net.w2, c.net.b2, c.net.w3, c.net.b3] == \
        [t.data_ptr() for i in (0, 4, 8) for t in (net[i].weight, net[i].bias)]
    assert [c.g1, c.be1, c.g2, c.be2] == [t.data_ptr() for i in (2, 6) for t in (net[i].weight, net[i].bias)]
    net[6].weight = torch.nn.Parameter(torch.ones(64)[::2], requires_grad=False)
    assert not net[6].weight.is_contiguous()
    with pytest.raises(droq.LearnError, match="contiguous float32"):
        d._critic_table(net)
    net[6].weight = torch.nn.Parameter(torch.ones(32, dtype=torch.float64), requires_grad=False)
    with pytest.raises(droq.LearnError, match="contiguous float32"):
        d._critic_table(net)


def _batch(B=32, A=3, seed=6):
    rng = np.random.default_rng(seed)
    return {"obs": torch.as_tensor(rng.normal(size=(B, 7)).astype(np.float32)),
            "action": torch.as_tensor(np.tanh(rng.normal(size=(B, A))).astype(np.float32)),
            "y": torch.as_tensor(rng.normal(size=B).astype(np.float32)),
            "mask": torch.as_tensor((rng.uniform(size=B) < 0.9).astype(np.float32))}


def test_one_gradient_step_changes_every_parameter_and_moves_the_targets_by_tau():
    d = _droq()
    batch = _batch()
    params = list(d.actor.parameters()) + [p for c in d.critics for p in c.parameters()] + [d.log_alpha]
    assert len(params) == 6 + 3 * 10 + 1
    before = [p.detach().clone() for p in params]
    t_before = [p.detach().clone() for t in d.targets for p in t.parameters()]
    stats = d.gradient_step(batch)
    assert set(stats) == {"critic_loss", "actor_loss", "alpha_loss", "alpha", "entropy", "masked"}
    assert all(bool(torch.isfinite(v).all()) for v in stats.values()), stats
    for b, a in zip(before, params):                                     # (LayerNorm's weights and biases are among them)
        assert bool((a != b).all()) and bool(torch.isfinite(a).all())
    src = [p.detach() for c in d.critics for p in c.parameters()]
    for tb, ta, s in zip(t_before, [p for t in d.targets for p in t.parameters()], src):
        assert torch.allclose(ta, tb + 0.25 * (s - tb), rtol=1e-6, atol=1e-7) and not torch.equal(ta, tb)
    assert all(c.training for c in d.critics)
    # a critic step alone leaves the actor and the temperature alone
    kept = [p.detach().clone() for p in list(d.actor.parameters()) + [d.log_alpha]]
    d.critic_step(batch)
    assert all(torch.equal(k, p) for k, p in zip(kept, list(d.actor.parameters()) + [d.log_alpha]))
    # with utd > 1 the launches of one gradient step are not the whole actor step
    with pytest.raises(droq.LearnError, match="utd > 1"):
        d.sample_and_target()


def test_state_dict_round_trip_and_the_mismatch_errors():
    d = _droq()
    batch = _batch()
    d.gradient_step(batch)
    sd = d.state_dict(include_replay=True)
    assert sd["droq"] == {"dropout": 0.25, "utd": 3, "ln_eps": 1e-5}
    assert set(sd["critics"][0]) == {"0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "6.weight", "6.bias",
                                     "8.weight", "8.bias"} == set(sd["targets"][2])
    kept = sd["critics"][1]["6.weight"].clone()
    d.gradient_step(batch)
    assert torch.equal(kept, sd["critics"][1]["6.weight"]) and not torch.equal(kept, d.critics[1][6].weight)
    again = _droq(seed=77)
    again.load_state_dict(sd)
    assert torch.equal(again.critics[1][6].weight, kept) and again.seed == 5
    assert all(torch.equal(sd["targets"][0][k], v) for k, v in again.targets[0].state_dict().items())
    # torch's dropout draws from the global generator: from the same state two learners take the same step
    torch.manual_seed(9)
    s1 = again.gradient_step(batch)
    d.load_state_dict(sd)
    torch.manual_seed(9)
    s2 = d.gradient_step(batch)
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    for kw, name in ((dict(dropout=0.5), "dropout"), (dict(utd=2), "utd"), (dict(ln_eps=1e-3), "ln_eps")):
        with pytest.raises(ValueError, match=f"written with {name}"):
            _droq(**kw).load_state_dict(sd)
    with pytest.raises(ValueError, match="written with dropout = nothing"):
        d.load_state_dict({k: v for k, v in sd.items() if k != "droq"})
