"""Host tests of populations (include/learn/rp_pop.h, robopianist_amd/population.py): the index maps of the twins
(tests/pop_reference.py) by brute force, the batched torch modules and one population gradient step against P separate
learners in float64, the independence of the members (bit for bit), the binding's symbols, struct sizes and argument
validation (refused calls return before anything touches a device), the class's own refusals, and the per-env musical
metrics of MidiEvaluationWrapper."""

from __future__ import annotations

import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pop_reference as popr  # noqa: E402
import sac_reference as sr  # noqa: E402
from test_offpolicy_host import _SpecEnv, _labelled_ring  # noqa: E402
from robopianist_amd import droq, learning, offpolicy, population  # noqa: E402

F_, M_, L_ = sr.FIRST, sr.MID, sr.LAST


# ---- the twins' index maps ---------------------------------------------------------------------------------------------
def test_layout_maps_are_partitions_of_the_array_rows():
    for P, rows in ((1, 5), (3, 17), (5, 1), (2, 33)):
        for layout in (popr.INTERLEAVED, popr.BLOCKED):
            seen = np.concatenate([popr.array_rows(p, P, rows, layout) for p in range(P)])
            assert sorted(seen.tolist()) == list(range(P * rows))
            for p in range(P):
                for j in range(rows):
                    want = p + P * j if layout == popr.INTERLEAVED else p * rows + j
                    assert popr.array_rows(p, P, rows, layout)[j] == want
                assert popr.array_rows(p, P, rows, layout, 1, rows - 1).tolist() == popr.array_rows(p, P, rows, layout)[1:].tolist()
        assert all((popr.array_rows(p, P, rows, popr.INTERLEAVED) % P == p).all() for p in range(P))


@pytest.mark.parametrize("C, E, n_written, P", [(4, 6, 3, 3), (5, 12, 13, 3), (3, 4, 9, 2), (5, 7, 13, 1), (6, 20, 1000, 5)])
def test_twin_sampler_draws_member_ps_rows_from_member_ps_envs(C, E, n_written, P):
    rng = np.random.default_rng(C * 100 + n_written + P)
    types_ = rng.choice(np.array([F_, M_, M_, M_, L_], np.int32), size=(n_written + 1, E))
    ring = _labelled_ring(C, E, n_written, lambda m, e: types_[m, e])
    n, Em = 150, E // P
    out = popr.sample(ring, n_written, P, n, seed=5, round_=n_written)
    Fc = min(n_written, C)
    for p in range(P):
        for b in range(p * n, (p + 1) * n):
            if out["mask"][b] == 0:
                assert out["index"][b] == -1 and out["tries"][b] == sr.TRIES + 1
                continue
            m, e = int(out["obs"][b, 0]), int(out["obs"][b, 1])           # (the ring's rows say where they come from)
            assert e % P == p and n_written - Fc <= m <= n_written - 2
            assert out["index"][b] == (m % C) * E + e
            assert out["next_obs"][b, 0] == m + 1 and out["next_obs"][b, 1] == e and out["action"][b, 1] == e
            assert out["reward"][b] == m + 1.25 and types_[m, e] != L_ and types_[m + 1, e] != F_
        # the remap, by brute force over every (slot, jj)
        for s in range(C):
            for jj in range(Em):
                assert popr.remap_index([s * Em + jj], p, P, E)[0] == s * E + p + P * jj
    assert popr.remap_index([-1], 0, P, E)[0] == -1
    # the draw is the header's: counter row p n + b over N = (F - 1) Em, then e = p + P jj
    for p in range(P):
        m, jj = sr.draw(n_written, C, Em, 5, n_written, np.arange(p * n, (p + 1) * n))
        ok = (ring["step_type"][m % C, p + P * jj] != L_) & (ring["step_type"][(m + 1) % C, p + P * jj] != F_)
        first = np.where(ok.any(1), ok.argmax(1), -1)
        rows = np.arange(p * n, (p + 1) * n)
        hit = first >= 0
        want = (m[hit, first[hit]] % C) * E + p + P * jj[hit, first[hit]]
        assert np.array_equal(out["index"][rows][hit], want) and (out["index"][rows][~hit] == -1).all()
    # for one member the twin is the single learner's on the ring itself, index included
    if P == 1:
        single = sr.sample(ring, n_written, n, 5, n_written)
        assert all(np.array_equal(out[k], single[k]) for k in single)
    # member and row sub-ranges leave the rest as it was
    base = {k: np.full_like(v, 9) for k, v in out.items() if k != "tries"}
    keys = list(base)                                                      # (the twin adds "tries" to the dict it is given)
    part = popr.sample(ring, n_written, P, n, 5, n_written, out=base, members=[P - 1], row_first=7, row_count=20)
    inside = np.zeros(P * n, bool); inside[(P - 1) * n + 7:(P - 1) * n + 27] = True
    for k in keys:
        assert np.array_equal(part[k][inside], out[k][inside]) and (part[k][~inside] == 9).all(), k


def test_twin_moments_rows_are_the_members_envs_in_slot_order():
    k, E, D, P = 3, 6, 2, 3
    obs = np.zeros((k, E, D), np.float32)
    obs[..., 0], obs[..., 1] = np.arange(k)[:, None], np.arange(E)[None, :]
    for p in range(P):
        rows = popr.member_slots(obs, p, P)
        Em = E // P
        for r in range(k * Em):
            t, jj = divmod(r, Em)
            assert rows[r].tolist() == [t, p + P * jj]


# ---- batched torch against per-member torch, float64 ----------------------------------------------------------------------
def _population(P=3, E=6, seed=5, **kw):
    args = dict(hidden=(16, 32), n_critics=2, capacity=4, batch_size=24, lr=1e-2, tau=0.25, seed=seed, dropout=0.0, utd=2)
    args.update(kw)
    return population.DroQPopulation(_SpecEnv(E, (4, 3), 3), P, **args)


def _double(pop):
    """The population's torch side in float64 (the parameters stay the optimizers')."""
    for net in [pop.actor] + pop.critics + pop.targets:
        net.double()
    pop.log_alpha.data = pop.log_alpha.data.double()
    pop.target_entropy, pop.gamma = pop.target_entropy.double(), pop.gamma.double()
    pop._mean_f32, pop._inv_std_f32 = pop._mean_f32.double(), pop._inv_std_f32.double()
    return pop


def _batch(P, B, D=7, A=3, seed=6, dtype=torch.float64):
    rng = np.random.default_rng(seed)
    t = lambda x: torch.as_tensor(x).to(dtype)
    mask = (rng.uniform(size=(P, B)) < 0.8).astype(np.float64)
    mask[:, 0] = 0.0                                                       # a masked row in every member
    return {"obs": t(rng.normal(size=(P, B, D))), "action": t(np.tanh(rng.normal(size=(P, B, A)))),
            "y": t(rng.normal(size=(P, B))), "mask": t(mask)}


def test_batched_forward_equals_the_members_own_sequentials():
    pop = _double(_population())
    with torch.no_grad():   # LayerNorm's parameters off 1 and 0, per member
        for c in pop.critics:
            for i in (2, 6):
                c[i].weight.uniform_(0.5, 1.5); c[i].bias.uniform_(-0.5, 0.5)
    x = _batch(pop.P, 24)
    xa = torch.cat([x["obs"], x["action"]], dim=2)
    with torch.no_grad():
        head, qs = pop.actor(x["obs"]), [c(xa) for c in pop.critics]
    assert tuple(head.shape) == (3, 24, 6) and tuple(qs[0].shape) == (3, 24, 1)
    for p in range(pop.P):
        actor = pop.actor_of(p)
        assert [type(m) for m in actor] == [nn.Linear, nn.Tanh, nn.Linear, nn.Tanh, nn.Linear]
        with torch.no_grad():
            assert float((actor(x["obs"][p]) - head[p]).abs().max()) <= 1e-12
            for c, q in zip(pop.critics, qs):
                net = population.member_network(c, p)
                assert [type(m) for m in net] == [nn.Linear, nn.Dropout, nn.LayerNorm, nn.ReLU, nn.Linear, nn.Dropout,
                                                  nn.LayerNorm, nn.ReLU, nn.Linear]
                assert float((net(xa[p]) - q[p]).abs().max()) <= 1e-12
        # a copy: writing to it leaves the population alone
        with torch.no_grad():
            actor[0].weight.add_(1.0)
        assert not torch.equal(actor[0].weight, pop.actor[0].weight[p])


def test_members_are_drawn_as_the_single_learner_draws_them():
    """Member after member under the forked generator: member 0 of any population, and the one member of P = 1, is
    droq.DroQ of the same seed; the global generator is left alone."""
    torch.manual_seed(123)
    state = torch.random.get_rng_state()
    pop = _population(P=3, seed=5)
    assert torch.equal(torch.random.get_rng_state(), state)
    single = droq.DroQ(_SpecEnv(6, (4, 3), 3), hidden=(16, 32), n_critics=2, capacity=4, batch_size=24, seed=5, dropout=0.0)
    for (k, a), b in zip(single.actor.state_dict().items(), pop.actor_of(0).state_dict().values()):
        assert torch.equal(a, b), k
    for c_single, c_pop in zip(single.critics, pop.critics):
        for (k, a), b in zip(c_single.state_dict().items(), population.member_network(c_pop, 0).state_dict().values()):
            assert torch.equal(a, b), k
    assert not torch.equal(pop.actor[0].weight[0], pop.actor[0].weight[1])
    for net in [pop.actor] + pop.critics + pop.targets:
        assert all(p.is_contiguous() and p.dtype == torch.float32 and p.shape[0] == 3 for p in net.parameters())
    assert tuple(pop.actor[0].weight.shape) == (3, 16, 7) and tuple(pop.critics[0][2].weight.shape) == (3, 16)
    assert all(not p.requires_grad for t in pop.targets for p in t.parameters())
    loaded = droq.DroQ(_SpecEnv(2, (4, 3), 3), hidden=(16, 32), n_critics=2, capacity=4, batch_size=24, seed=9)
    loaded.actor.load_state_dict(pop.actor_of(2).state_dict())
    assert torch.equal(loaded.actor[4].bias, pop.actor[4].bias[2])


def test_one_population_step_equals_p_separate_steps_with_offpolicys_losses():
    P, B, A, lr_, tau = 3, 24, 3, 1e-2, 0.25
    pop = _double(_population(P=P, gamma=[0.9, 0.95, 0.99], init_alpha=[0.1, 0.5, 2.0], target_entropy=[-3.0, -1.0, -2.0]))
    batch = _batch(P, B)
    members = []
    for p in range(P):
        actor = pop.actor_of(p)
        critics = [population.member_network(c, p) for c in pop.critics]
        targets = [population.member_network(t, p) for t in pop.targets]
        log_alpha = nn.Parameter(pop.log_alpha.detach()[p:p + 1].clone())
        adam = lambda ps: torch.optim.Adam(ps, lr=lr_)
        members.append((actor, critics, targets, log_alpha, adam(list(actor.parameters())),
                        adam([q for c in critics for q in c.parameters()]), adam([log_alpha])))
    gen_state = pop._gen.get_state()
    lc = pop.critic_step(batch)
    stats = pop.actor_step(batch)
    g = torch.Generator()
    g.set_state(gen_state)
    eps = torch.randn(P, B, A, generator=g, dtype=torch.float64)
    for p, (actor, critics, targets, log_alpha, opt_a, opt_c, opt_t) in enumerate(members):
        b = {k: v[p] for k, v in batch.items()}
        xn = torch.clamp((b["obs"] - pop._mean_f32[p]) * pop._inv_std_f32[p], -pop.obs_clip, pop.obs_clip)
        xa = torch.cat([xn, b["action"]], dim=1)
        loss_c = offpolicy.critic_loss([c(xa).squeeze(-1) for c in critics], b["y"], b["mask"])
        opt_c.zero_grad(); loss_c.backward(); opt_c.step()
        with torch.no_grad():
            for t, c in zip(targets, critics):
                for tp, cp in zip(t.parameters(), c.parameters()):
                    tp.lerp_(cp, tau)
        a_new, logp_new, _ = offpolicy.squashed_gaussian(actor(xn), eps[p], pop.log_std_bounds)
        xa_new = torch.cat([xn, a_new], dim=1)
        q_new = torch.stack([c(xa_new).squeeze(-1) for c in critics]).min(0).values
        loss_a = offpolicy.actor_loss(log_alpha, logp_new, q_new, b["mask"])
        opt_a.zero_grad(); loss_a.backward(); opt_a.step()
        loss_t = offpolicy.alpha_loss(log_alpha, logp_new, float(pop.target_entropy[p]), b["mask"])
        opt_t.zero_grad(); loss_t.backward(); opt_t.step()
        close = lambda x, y: float((x.detach() - y.detach()).abs().max()) <= 1e-12
        assert close(lc[p], loss_c) and close(stats["actor_loss"][p], loss_a) and close(stats["alpha_loss"][p], loss_t)
        assert close(pop.log_alpha[p], log_alpha[0]) and not close(pop.log_alpha[p], torch.tensor(np.log([0.1, 0.5, 2.0][p])))
        for mine, theirs in zip(pop.actor_of(p).parameters(), actor.parameters()):
            assert close(mine, theirs)
        for group, others in ((pop.critics, critics), (pop.targets, targets)):
            for net, other in zip(group, others):
                for mine, theirs in zip(population.member_network(net, p).parameters(), other.parameters()):
                    assert close(mine, theirs)
    # the population's own loss functions are the sums of offpolicy's over the members
    q = [torch.randn(P, B, dtype=torch.float64) for _ in range(2)]
    want = sum(offpolicy.critic_loss([x[p] for x in q], batch["y"][p], batch["mask"][p]) for p in range(P))
    assert abs(float(population.critic_loss(q, batch["y"], batch["mask"]) - want)) <= 1e-12
    la = pop.log_alpha.detach()
    want = sum(offpolicy.actor_loss(la[p], q[0][p], q[1][p], batch["mask"][p]) for p in range(P))
    assert abs(float(population.actor_loss(la, q[0], q[1], batch["mask"]) - want)) <= 1e-12
    want = sum(offpolicy.alpha_loss(la[p], q[0][p], float(pop.target_entropy[p]), batch["mask"][p]) for p in range(P))
    assert abs(float(population.alpha_loss(la, q[0], pop.target_entropy, batch["mask"]) - want)) <= 1e-12


def _member_state(pop, p):
    nets = [pop.actor] + pop.critics + pop.targets
    return [t.detach()[p].clone() for net in nets for t in net.parameters()] + [pop.log_alpha.detach()[p].clone()]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_member_0_does_not_see_member_1s_rows_gamma_or_temperature(dtype):
    kw = dict(P=3, dropout=0.25)
    a, b = _population(**kw), _population(gamma=[0.99, 0.5, 0.99], init_alpha=[1.0, 0.05, 1.0], **kw)
    if dtype == torch.float64:
        _double(a), _double(b)
    batch_a = _batch(3, 24, dtype=dtype)
    other = _batch(3, 24, seed=99, dtype=dtype)
    batch_b = {k: torch.stack([v[0], other[k][1], v[2]]) for k, v in batch_a.items()}
    before = _member_state(a, 0)
    for pop, batch in ((a, batch_a), (b, batch_b)):
        torch.manual_seed(3)   # (torch's dropout draws from the global generator)
        for _ in range(2):
            pop.critic_step(batch)
            pop.actor_step(batch)
    for p in (0, 2):
        for x, y in zip(_member_state(a, p), _member_state(b, p)):
            assert torch.equal(x, y)
    assert all(not torch.equal(x, y) for x, y in zip(before, _member_state(a, 0)))
    assert not any(torch.equal(x, y) for x, y in zip(_member_state(a, 1), _member_state(b, 1)))


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_dims_and_struct_sizes():
    L = population.load_library()
    assert set(population.EXPORTED_SYMBOLS) == {"rp_pop_act", "rp_pop_sample", "rp_pop_target", "rp_pop_moments",
                                                "rp_pop_dim", "rp_pop_last_error"}
    assert [getattr(L, s) for s in population.EXPORTED_SYMBOLS]
    assert population.dim("interleaved") == population.INTERLEAVED == popr.INTERLEAVED == 0
    assert population.dim("blocked") == population.BLOCKED == popr.BLOCKED == 1
    assert population.dim("tile_major") == population.TILE_MAJOR and population.dim("member_major") == population.MEMBER_MAJOR
    assert population.dim("default_grid_order") in (population.TILE_MAJOR, population.MEMBER_MAJOR)
    assert population.dim("tile_rows") == offpolicy.dim("tile_rows") == 16
    assert population.dim("max_critics") == droq.MAX_CRITICS == 4 and population.dim("sample_tries") == offpolicy.SAMPLE_TRIES
    assert population.dim("max_hidden") == learning.MAX_HIDDEN and population.dim("max_actions") == learning.MAX_ACTIONS
    assert population.dim("moment_lanes") == learning.dim("moment_lanes") and population.dim("nothing") == -1
    # the layouts of the header on the LP64 ABI
    assert [ctypes.sizeof(population._ARGS[k]) for k in ("act", "sample", "target", "moments")] == [168, 176, 208, 96]
    for entry in ("act", "sample", "target", "moments"):
        a = population.make_args(entry)
        assert population.call_raw(entry, a) != 0 and "struct_size" not in population.last_error()
        a.struct_size -= 8
        assert population.call_raw(entry, a) != 0 and "struct_size" in population.last_error()
    # each library keeps its own symbols
    assert not hasattr(droq.load_library(), "rp_pop_target") and not hasattr(L, "rp_droq_target")
    assert not hasattr(L, "rp_sac_act") and not hasattr(L, "rp_learn_moments")


_A = 0x1000   # a non-null address: a refused call never reads it


def _refused(entry, match, **values):
    assert population.call_raw(entry, population.make_args(entry, **values)) != 0
    assert match in population.last_error(), population.last_error()
    assert population.last_error().startswith(f"rp_pop_{entry}: ")


def _accepted(entry, **values):
    assert population.call_raw(entry, population.make_args(entry, **values)) == 0, population.last_error()


def test_argument_validation_refuses_before_any_launch():
    mlp = learning.Mlp(*([_A] * 6))
    act = dict(obs=_A, mean=_A, inv_std=_A, obs_clip=5.0, log_std_min=-5.0, log_std_max=2.0, actor=ctypes.pointer(mlp),
               action=_A, logp=_A, precision=64, D=3, H1=16, H2=32, A=2, P=3, rows=4, layout=population.INTERLEAVED,
               grid_order=population.TILE_MAJOR, member_first=0, member_count=3, row_first=0, row_count=4)
    smp = dict(ring_obs=_A, ring_action=_A, ring_reward=_A, ring_discount=_A, ring_step_type=_A, obs=_A, next_obs=_A,
               action=_A, reward=_A, discount=_A, mask=_A, index=_A, n_written=5, C=4, E=6, D=3, A=2, P=3, n=8,
               member_first=0, member_count=3, row_first=0, row_count=8)
    c = droq.Critic(mlp, _A, _A, _A, _A)
    tgt = dict(next_obs=_A, action=_A, logp=_A, reward=_A, discount=_A, mean=_A, inv_std=_A, obs_clip=5.0, gamma=_A,
               log_alpha=_A, critics=droq.critic_table([c, c]), n_critics=2, y=_A, drop_threshold=0, keep_scale=1.0,
               ln_eps=1e-5, D=3, H1=16, H2=32, A=2, P=3, n=8, grid_order=population.MEMBER_MAJOR, member_first=0,
               member_count=3, row_first=0, row_count=8)
    mom = dict(obs=_A, mean=_A, M2=_A, mean_f32=_A, inv_std_f32=_A, count=0.0, eps=1e-8, k=2, E=6, D=3, P=3, member_first=0,
               member_count=3)
    blocks = {"act": act, "sample": smp, "target": tgt, "moments": mom}
    # what is the population's own
    for entry, ok in blocks.items():
        for P in (0, -1):
            _refused(entry, "P must be >= 1", **dict(ok, P=P))
        for first, count in ((0, 4), (3, 1), (-1, 1), (2, 2), (0, -1)):
            _refused(entry, "the member range", **dict(ok, member_first=first, member_count=count))
        _accepted(entry, **dict(ok, member_first=3, member_count=0))        # no member: nothing is launched
    for entry in ("sample", "moments"):
        _refused(entry, "is not a multiple of P", **dict(blocks[entry], E=7))
        _refused(entry, "is not a multiple of P", **dict(blocks[entry], E=4))
    for layout in (2, -1):
        _refused("act", "layout must be", **dict(act, layout=layout))
    for entry in ("act", "target"):
        _refused(entry, "grid_order must be", **dict(blocks[entry], grid_order=2))
    for entry, name in (("act", "rows"), ("sample", "n"), ("target", "n")):
        ok = blocks[entry]
        _refused(entry, f"{name} must be >= 1", **dict(ok, **{name: 0, "row_count": 0}))
        _refused(entry, "the row range", **dict(ok, row_first=1))
        _refused(entry, "the row range", **dict(ok, row_first=-1, row_count=1))
        _refused(entry, "must be < 2^31", **dict(ok, **{name: 2 ** 30}))
        _accepted(entry, **dict(ok, row_count=0))                          # no row: nothing is launched
    _refused("sample", "(C - 1) E / P must be < 2^32", **dict(smp, C=2 ** 31 - 1, E=2 ** 31 - 1, P=1, member_count=1, n=8))
    _refused("moments", "k must be >= 1", **dict(mom, k=0))
    # what the single-learner entry points refuse, under this library's names
    for name in ("obs", "mean", "inv_std", "action"):
        _refused("act", "a pointer is NULL", **dict(act, **{name: None}))
    _refused("act", "actor is NULL", **dict(act, actor=None))
    _refused("act", "a sampling actor needs logp", **dict(act, logp=None))
    _accepted("act", **dict(act, logp=None, deterministic=1, row_count=0))
    _refused("act", "H1 must be", **dict(act, H1=24))
    _refused("act", "A must be", **dict(act, A=129))
    _refused("act", "the actor has a NULL", **dict(act, actor=ctypes.pointer(learning.Mlp(_A, _A, None, _A, _A, _A))))
    for name in ("ring_obs", "ring_step_type", "obs", "mask"):
        _refused("sample", "a pointer is NULL", **dict(smp, **{name: None}))
    _refused("sample", "C must be >= 2", **dict(smp, C=1))
    _refused("sample", "n_written must be >= 2", **dict(smp, n_written=1))
    _accepted("sample", **dict(smp, index=None, row_count=0))
    for name in ("next_obs", "logp", "mean", "gamma", "log_alpha", "y"):
        _refused("target", "a pointer is NULL", **dict(tgt, **{name: None}))
    _refused("target", "critics is NULL", **dict(tgt, critics=None))
    _refused("target", "n_critics", **dict(tgt, n_critics=5))
    _refused("target", "keep_scale must be > 0", **dict(tgt, keep_scale=0.0))
    _refused("target", "the LayerNorm of critic 1 has a NULL",
             **dict(tgt, critics=droq.critic_table([c, droq.Critic(mlp, _A, None, _A, _A)])))
    for name in ("obs", "mean", "M2", "mean_f32", "inv_std_f32"):
        _refused("moments", "a pointer is NULL", **dict(mom, **{name: None}))
    _refused("moments", "count must be >= 0", **dict(mom, count=-1.0))
    _refused("moments", "eps must be > 0", **dict(mom, eps=0.0))
    with pytest.raises(TypeError):
        population.make_args("act", nothing=1)
    # the module functions raise the library's message
    with pytest.raises(population.LearnError, match="is not a multiple of P"):
        population.moments(_A, _A, _A, _A, _A, 0.0, 1e-8, 1, 7, 3, 2)


# ---- the class ---------------------------------------------------------------------------------------------------------
def test_constructor_refusals_and_per_member_hyper_parameters():
    with pytest.raises(ValueError, match="does not divide n_envs"):
        _population(P=4, E=6)
    with pytest.raises(ValueError, match="members must be >= 1"):
        _population(P=0)
    for name in ("gamma", "init_alpha", "target_entropy"):
        for bad in ([0.5, 0.6], [0.5] * 4):
            with pytest.raises(ValueError, match=f"{name} must be a scalar or a sequence of 3"):
                _population(**{name: bad})
    for kw, match in ((dict(dropout=1.0), "dropout"), (dict(utd=0), "utd"), (dict(ln_eps=0.0), "ln_eps"),
                      (dict(hidden=(20, 32)), "multiples of 16"), (dict(n_critics=5), "n_critics"),
                      (dict(capacity=1), "capacity"), (dict(batch_size=0), "batch_size")):
        with pytest.raises(ValueError, match=match):
            _population(**kw)
    pop = _population(gamma=[0.9, 0.95, 0.99], init_alpha=0.5, target_entropy=None)
    assert isinstance(pop, learning.DeviceLearner) and (pop.P, pop.Em, pop.members) == (3, 2, 3)
    np.testing.assert_allclose(pop.gamma.numpy(), np.float32([0.9, 0.95, 0.99]))
    np.testing.assert_allclose(pop.alpha, [0.5] * 3, rtol=1e-6)
    assert pop.target_entropy.tolist() == [-3.0] * 3 and tuple(pop.log_alpha.shape) == (3,)
    # batch_size is per member: the buffers hold P x utd x B rows, a member's ranges side by side
    assert tuple(pop._u_obs.shape) == (3 * 2 * 24, 7) and tuple(pop.rows()["obs"].shape) == (3, 48, 7)
    assert tuple(pop.minibatch()["y"].shape) == (3, 24) and pop.minibatch()["y"].data_ptr() == pop._u_y[24:].data_ptr()
    assert tuple(pop.normalizer[1].shape) == (3, 7) and pop.normalizer_of(2)[3].data_ptr() == pop.normalizer[3][2].data_ptr()
    with pytest.raises(population.LearnError, match="collect"):
        pop.update()
    with pytest.raises(ValueError, match="member 3 of 3"):
        pop.actor_of(3)
    pop.actor[0].weight = nn.Parameter(torch.ones(3, 16, 14)[:, :, ::2])
    with pytest.raises(population.LearnError, match="contiguous float32"):
        pop._actor_table()


def test_state_dict_round_trip_and_the_mismatch_errors():
    pop = _population(gamma=[0.9, 0.95, 0.99])
    batch = _batch(3, 24, dtype=torch.float32)
    pop.critic_step(batch); pop.actor_step(batch)
    sd = pop.state_dict(include_replay=True)
    assert sd["members"] == 3 and sd["droq"] == {"dropout": 0.0, "utd": 2, "ln_eps": 1e-5}
    assert tuple(sd["actor"]["0.weight"].shape) == (3, 16, 7) and tuple(sd["normalizer"]["mean"].shape) == (3, 7)
    kept = sd["critics"][1]["6.weight"].clone()
    pop.critic_step(batch)
    assert torch.equal(kept, sd["critics"][1]["6.weight"]) and not torch.equal(kept, pop.critics[1][6].weight)
    again = _population(seed=77)
    again.load_state_dict(sd)
    assert torch.equal(again.critics[1][6].weight, kept) and again.seed == 5 and again.gamma.tolist() == pop.gamma.tolist()
    s1, s2 = again.actor_step(batch), None
    pop.load_state_dict(sd)
    s2 = pop.actor_step(batch)
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    with pytest.raises(ValueError, match="written with members = 3, this population has members = 2"):
        _population(P=2).load_state_dict(sd)
    with pytest.raises(ValueError, match="written with members = nothing"):
        pop.load_state_dict({k: v for k, v in sd.items() if k != "members"})
    with pytest.raises(ValueError, match="written with utd"):
        _population(utd=3).load_state_dict(sd)


# ---- the per-env musical metrics ----------------------------------------------------------------------------------------
def test_per_env_musical_metrics_average_to_the_wrappers_own_and_are_nan_before_an_episode_ends():
    from test_tasks_host import _get_env
    from robopianist_amd import music
    from robopianist_amd.music import midi_file
    from robopianist_amd.wrappers import MidiEvaluationWrapper
    midis = [music.load("CMajorScaleTwoHands"), music.load("CMajorChordProgressionTwoHands")]   # 151 and 81 steps
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = MidiEvaluationWrapper(_get_env(n_envs=4, control_timestep=0.05, midi=midis), deque_size=2)
    names = ["precision", "recall", "f1", "sustain_precision", "sustain_recall", "sustain_f1"]
    env.reset()
    assert all(bool(torch.isnan(v).all()) for v in env.get_musical_metrics_per_env().values())
    rng = np.random.default_rng(0)
    lo, hi = env.action_spec().minimum, env.action_spec().maximum

    def check(finished):
        per = env.get_musical_metrics_per_env()
        assert list(per) == names and all(tuple(v.shape) == (4,) and v.dtype == torch.float64 for v in per.values())
        n = np.minimum(np.asarray(finished), 2)
        for k, want in env.get_musical_metrics().items():
            v = per[k].numpy()
            assert np.array_equal(np.isnan(v), n == 0), (k, v, n)
            assert abs(np.nansum(v * n) / n.sum() - want) <= 1e-12, k
        return per

    piano = env.task.piano
    key = midi_file.note_name_to_key_number("C4")
    qmax = piano._qpos_range[key, 1].item()

    def step():
        env.physics.qpos[3, piano.joints[key]] = qmax                      # env 3 holds a key down, the others none
        env.step(rng.uniform(lo, hi, (4,) + lo.shape))

    for t in range(1, 101):
        step()
    first = check([0, 1, 0, 1])                     # the short song's envs have ended once, the others never
    assert first["f1"][1] != first["f1"][3]         # the envs' own numbers, not a batch mean
    for t in range(101, 260):
        step()
    check([1, 3, 1, 3])                             # (the deque holds two episodes)
