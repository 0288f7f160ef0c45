"""GPU tests of the population's fused critic step (include/learn/rp_pop_critic.h) and of
population.DroQPopulation(critic_step="fused").

The bar is bits: member p's q rows, its ten gradients and its p, m, v and target tensors after `pop_critic.step` equal
what `critic.step` (librp_critic.so) leaves when called on the same arrays of P n rows with B = P n, row_first =
p n + row_first and member p's slices -- the two libraries run one device text.  Member 0 of the first test holds
critic_cases' own problem at the array rows [0, R), so its dropout masks are the ones the case's seed was conditioned
under, and is held to the float64 twin as well, under test_gpu_critic's bar (8 float32 restatement errors per tensor).
The lines of a run are kept in profiles/pop_critic_gpu_tests.txt.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_cases as cc  # noqa: E402
import critic_reference as cr  # noqa: E402
from test_gpu_offpolicy import POISON, _dev, _piano_env, _same_bits, _stream, _up  # noqa: E402
from test_gpu_population import TOY, _MemberToyEnv  # noqa: E402
from robopianist_amd import critic, pop_critic, population  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = ("obs", "action", "y", "mask")
KINDS = ("p", "m", "v", "target")
ORDERS = (pop_critic.TILE_MAJOR, pop_critic.MEMBER_MAJOR)


def _member_problem(case, p):
    """Member 0: the case's own problem; the others: the same case drawn with other seeds."""
    return cc.problem(case) if p == 0 else cc.problem(case, cc.SEEDS[case] + 1000 * p)


class _Batch:
    """The host arrays of a population of P members with n rows each (blocked) and its stacked tensors: member p holds
    `problems[p]`'s rows at its rows [first, first + R) -- every other row is NaN -- and its networks, m and v.
    `override[p]`: arrays that replace the problem's (rows) for member p."""

    def __init__(self, case, problems, k, mode, n, first=0, override=None):
        R, D, H1, H2, A, _ = case
        self.case, self.P, self.k, self.mode, self.n, self.first, self.R = case, len(problems), k, mode, n, first, R
        self.md = problems[0].mode[mode]
        shape = {"obs": (D,), "action": (A,), "y": (), "mask": ()}
        self.rows = {key: np.full((self.P * n,) + shape[key], np.nan, np.float32) for key in ROWS}
        for p, pr in enumerate(problems):
            kw = dict(pr.kw, **((override or {}).get(p, {})))
            for key in ROWS:
                self.rows[key][p * n + first:p * n + first + R] = kw[key]
        self.mean = np.stack([pr.kw["mean"] for pr in problems])
        self.inv_std = np.stack([pr.kw["inv_std"] for pr in problems])
        groups = lambda pr: {"p": pr.kw["critics"], "m": pr.mode[mode]["m"], "v": pr.mode[mode]["v"], "target": pr.kw["targets"]}
        # kind -> critic -> ten stacked arrays [P][...]
        self.stacked = {kind: [[np.stack([groups(pr)[kind][i][t] for pr in problems]) for t in range(10)] for i in range(k)]
                        for kind in KINDS}

    def upload(self):
        d = {key: _up(v) for key, v in self.rows.items()}
        d["mean"], d["inv_std"] = _up(self.mean), _up(self.inv_std)
        return d


def _common(b):
    md = b.md
    return dict(eps=cc.EPS, betas=cc.BETAS, tau=cc.TAU, threshold=md["threshold"], keep_scale=md["keep_scale"], ln_eps=cc.LN_EPS,
                seed=cc.SEED, round_=cc.ROUND, hip_stream=_stream())


def _host(group):
    return [[t.cpu().numpy() for t in net] for net in group]


def _run_pop(b, order=None, members=None, launches=(pop_critic.STEP,)):
    """`pop_critic.step` on batch b -> {"q" [k][P n], "grad", "p", "m", "v", "target": critic -> ten arrays [P][...]}.
    `members`: (first, count); `launches`: the `launches` of successive calls on the same tensors and workspace (with
    more than one -> the list of the results after each call)."""
    _, D, H1, H2, A, _ = b.case
    dev, k, P, n = _dev(), b.k, b.P, b.n
    d = b.upload()
    T = {kind: [[_up(a) for a in net] for net in b.stacked[kind]] for kind in KINDS}
    G = [[torch.full_like(t, POISON) for t in net] for net in T["p"]]
    q = torch.full((k, P * n), POISON, device=dev)
    m_first, m_count = (0, P) if members is None else members
    nbytes = pop_critic.workspace_bytes(k, H1, H2, b.R, m_count)
    assert nbytes == m_count * critic.workspace_bytes(k, H1, H2, b.R)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device=dev)
    sets = lambda group: [critic.set_entry(net) for net in group]
    outs = []
    for launch in launches:
        pop_critic.step(d["obs"].data_ptr(), d["action"].data_ptr(), d["y"].data_ptr(), d["mask"].data_ptr(),
                        d["mean"].data_ptr(), d["inv_std"].data_ptr(), cc.CLIP, sets(T["p"]), sets(T["m"]), sets(T["v"]),
                        sets(T["target"]), q.data_ptr(), ws.data_ptr(), nbytes, D, H1, H2, A, P, n, b.md["step_size"],
                        b.md["bc2_sqrt"], grad=sets(G), member_first=m_first, member_count=m_count, row_first=b.first,
                        row_count=b.R, grid_order=order, launches=launch, **_common(b))
        torch.cuda.synchronize()
        out = {kind: _host(T[kind]) for kind in KINDS}
        out.update(q=q.cpu().numpy(), grad=_host(G))
        outs.append(out)
    return outs[0] if len(outs) == 1 else outs


def _run_single(b, p):
    """`critic.step` on the same arrays for member p: B = P n, row_first = p n + first, member p's slices."""
    _, D, H1, H2, A, _ = b.case
    dev, k, P, n = _dev(), b.k, b.P, b.n
    d = b.upload()
    T = {kind: [[_up(a[p]) for a in net] for net in b.stacked[kind]] for kind in KINDS}
    G = [[torch.full_like(t, POISON) for t in net] for net in T["p"]]
    q = torch.full((k, P * n), POISON, device=dev)
    nbytes = critic.workspace_bytes(k, H1, H2, b.R)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device=dev)
    sets = lambda group: [critic.set_entry(net) for net in group]
    critic.step(d["obs"].data_ptr(), d["action"].data_ptr(), d["y"].data_ptr(), d["mask"].data_ptr(),
                d["mean"][p].data_ptr(), d["inv_std"][p].data_ptr(), cc.CLIP, sets(T["p"]), sets(T["m"]), sets(T["v"]),
                sets(T["target"]), q.data_ptr(), ws.data_ptr(), nbytes, D, H1, H2, A, P * n, b.md["step_size"], b.md["bc2_sqrt"],
                grad=sets(G), row_first=p * n + b.first, row_count=b.R, **_common(b))
    torch.cuda.synchronize()
    out = {kind: _host(T[kind]) for kind in KINDS}
    out.update(q=q.cpu().numpy(), grad=_host(G))
    return out


def _member_rows(b, p):
    return slice(p * b.n + b.first, p * b.n + b.first + b.R)


def _differing(b, got, p, single):
    """The outputs of member p in `got` (a population result) whose bits are not `single`'s (critic.step's)."""
    r = _member_rows(b, p)
    bad = [] if _same_bits(got["q"][:, r], single["q"][:, r]) else ["q"]
    for kind in KINDS + ("grad",):
        for i in range(b.k):
            bad += [f"{kind}{i}.{name}" for t, name in enumerate(cr.PARAMS) if not _same_bits(got[kind][i][t][p], single[kind][i][t])]
    return bad


def _untouched(b, got, p):
    """The tensors of member p that are not what was uploaded (the gradients: POISON), and whether its q rows are POISON."""
    bad = [f"{kind}{i}.{name}" for kind in KINDS for i in range(b.k) for t, name in enumerate(cr.PARAMS)
           if not _same_bits(got[kind][i][t][p], b.stacked[kind][i][t][p])]
    bad += [f"grad{i}.{name}" for i in range(b.k) for t, name in enumerate(cr.PARAMS) if not (got["grad"][i][t][p] == POISON).all()]
    return bad + ([] if (got["q"][:, p * b.n:(p + 1) * b.n] == POISON).all() else ["q"])


def _flat_member(b, got, p):
    """Member p of a population result under critic_cases' keys."""
    return cc.flat({"q": got["q"][:, _member_rows(b, p)], **{kind: [[a[p] for a in net] for net in got[kind]]
                                                              for kind in KINDS + ("grad",)}})


def _within(got, ref, err32, label):
    pairs = {k: (float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()), err32[k]) for k in ref}
    ratio = lambda k: pairs[k][0] / pairs[k][1] if pairs[k][1] > 0 else (np.inf if pairs[k][0] > 0 else 0.0)
    worst = max(pairs, key=ratio)
    print(f"{label}: kernel error | float32 restatement error: q0 {pairs['q0'][0]:.2e} | {pairs['q0'][1]:.2e}, "
          f"p0.w1 {pairs['p0.w1'][0]:.2e} | {pairs['p0.w1'][1]:.2e} (worst ratio: {worst} {ratio(worst):.3f})")
    for k, (e, bar) in pairs.items():
        assert got[k].shape == ref[k].shape and e <= 8 * bar, (label, k, e, bar)


# ---- 1. bit for bit against the single-learner kernel ------------------------------------------------------------------
@pytest.mark.parametrize("case", [cc.CASES[1], cc.CASES[4], cc.WIDE_CASES[2]], ids=cc.case_id)
def test_every_member_has_the_bits_of_the_single_learners_step(case):
    R = case[0]
    n = R + 3                                                                # p n is no multiple of the tile
    for P in (1, 3):
        problems = [_member_problem(case, p) for p in range(P)]
        for k in (1, 3):
            for mode in ("on", "off"):
                b = _Batch(case, problems, k, mode, n)
                singles = [_run_single(b, p) for p in range(P)]
                inside = np.zeros(P * n, bool)
                for p in range(P):
                    inside[_member_rows(b, p)] = True
                for order in ORDERS:
                    got = _run_pop(b, order)
                    label = f"population step {case} P {P} critics {k} dropout {mode} order {order}"
                    for p in range(P):
                        assert _differing(b, got, p, singles[p]) == [], (label, p)
                    assert (got["q"][:, ~inside] == POISON).all() and np.isfinite(got["q"][:, inside]).all()
                    assert all(np.isfinite(a).all() for kind in KINDS + ("grad",) for net in got[kind] for a in net)
                    # every member steps: nothing keeps its uploaded bits
                    assert all(not np.array_equal(got[kind][i][t][p], b.stacked[kind][i][t][p])
                               for kind in KINDS for i in range(k) for t in range(10) for p in range(P))
                    # member 0 is the case's own problem on its own rows: the float64 twin's bar
                    _within(_flat_member(b, got, 0), cc.first(problems[0].ref[mode], k), problems[0].err32[mode], label)
                if P > 1:                                                    # the members differ, and so do their steps
                    assert not np.array_equal(got["p"][0][0][0], got["p"][0][0][1])


# ---- 2. ranges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [cc.CASES[1], cc.CASES[4]], ids=cc.case_id)
def test_member_and_row_ranges_read_and_write_nothing_outside(case):
    R, P, k = case[0], 4, 2
    n, first = R + 9, 5
    problems = [_member_problem(case, p) for p in range(P)]
    nan = _Batch(case, problems, k, "on", n, first)
    # the members outside the range: their rows are NaN everywhere, their tensors are looked at below
    for p in (0, 3):
        for key in ROWS:
            nan.rows[key][p * n:(p + 1) * n] = np.nan
    assert all(np.isnan(nan.rows["y"][p * n:(p + 1) * n]).sum() == (n if p in (0, 3) else n - R) for p in range(P))
    for order in ORDERS:
        got = _run_pop(nan, order, members=(1, 2))
        for p in (0, 3):
            assert _untouched(nan, got, p) == [], (order, p)
        for p in (1, 2):
            assert _differing(nan, got, p, _run_single(nan, p)) == [], (order, p)
            r = _member_rows(nan, p)
            outside = np.ones(n, bool); outside[first:first + R] = False
            assert (got["q"][:, p * n:(p + 1) * n][:, outside] == POISON).all() and np.isfinite(got["q"][:, r]).all()
            assert all(np.isfinite(got[kind][i][t][p]).all() for kind in KINDS + ("grad",) for i in range(k) for t in range(10))
    # a range of no member or no row launches nothing
    for members, rows in (((2, 0), R), ((0, 4), 0)):
        empty = _Batch(case, problems, k, "on", n, first)
        empty.R = rows
        got = _run_pop(empty, members=members)
        assert all(_untouched(empty, got, p) == [] for p in range(P))


# ---- 3. independence -----------------------------------------------------------------------------------------------------
def test_member_0_does_not_see_anything_of_member_1():
    case, k = cc.CASES[4], 2
    n = case[0] + 3
    a = _Batch(case, [_member_problem(case, 0), _member_problem(case, 1)], k, "on", n)
    b = _Batch(case, [_member_problem(case, 0), _member_problem(case, 2)], k, "on", n)
    b.rows["mask"][n:n + case[0]] = 1.0                                      # (another mask sum too)
    # everything of member 1 differs: rows, y, mask, mean and all four weight sets
    assert all(not np.array_equal(a.rows[key][n:n + case[0]], b.rows[key][n:n + case[0]]) for key in ROWS)
    assert not np.array_equal(a.mean[1], b.mean[1]) and not np.array_equal(a.inv_std[1], b.inv_std[1])
    assert all(not np.array_equal(a.stacked[kind][i][t][1], b.stacked[kind][i][t][1]) for kind in KINDS for i in range(k) for t in range(10))
    for order in ORDERS:
        ga, gb = _run_pop(a, order), _run_pop(b, order)
        fa, fb = _flat_member(a, ga, 0), _flat_member(b, gb, 0)
        assert [key for key in fa if not _same_bits(fa[key], fb[key])] == []
        f1a, f1b = _flat_member(a, ga, 1), _flat_member(b, gb, 1)
        assert all(not np.array_equal(f1a[key], f1b[key]) for key in f1a)


# ---- 4. M is per member ------------------------------------------------------------------------------------------------------
def test_the_mask_sum_is_each_members_own():
    case, k, P = cc.CASES[4], 2, 3
    R = case[0]
    n = R + 3
    problems = [_member_problem(case, p) for p in range(P)]
    quarter = np.zeros(R, np.float32)
    quarter[[1, 33, 69]] = 0.25                                              # MSUM = 0.75: M = 1, not 0.75
    assert cr.mask_sum(quarter) == np.float32(0.75)
    b = _Batch(case, problems, k, "on", n, override={1: dict(mask=np.zeros(R, np.float32)), 2: dict(mask=quarter)})
    md = b.md
    sc = [np.float32(md[key]) for key in ("step_size", "bc2_sqrt", "eps", "omb1", "beta2", "omb2", "tau")]
    for order in ORDERS:
        got = _run_pop(b, order)
        # member 0 steps as in the first test: an M summed over the launch's rows would move it off the twin
        assert _differing(b, got, 0, _run_single(b, 0)) == []
        _within(_flat_member(b, got, 0), cc.first(problems[0].ref["on"], k), problems[0].err32["on"], f"member 0 of 3, order {order}")
        # member 1, all masked: Adam on a zero gradient (M clamps to 1: 0 / 1, not 0 / 0)
        for i in range(k):
            for t, name in enumerate(cr.PARAMS):
                g = got["grad"][i][t][1]
                assert not g.any(), name
                want = cr.adam(b.stacked["p"][i][t][1], b.stacked["m"][i][t][1], b.stacked["v"][i][t][1], b.stacked["target"][i][t][1],
                               np.zeros_like(g), *sc)
                for kind, w in zip(KINDS, want):
                    assert _same_bits(got[kind][i][t][1], w), (kind, i, name)
        assert np.isfinite(got["q"][:, _member_rows(b, 1)]).all()
        # member 2, a mask sum of 0.75: M = 1, the twin's on its rows (dropout words of the absolute rows 2 n + j)
        assert _differing(b, got, 2, _run_single(b, 2)) == []
        kw = dict(problems[2].kw, critics=problems[2].kw["critics"][:k], targets=problems[2].kw["targets"][:k],
                  **{key: b.rows[key] for key in ROWS})
        run = lambda **o: cc.flat(cr.step(**kw, **problems[2].mode["on"], row_first=2 * n, row_count=R, **o), k)
        ref = run(dtype=np.float64)
        f2 = _flat_member(b, got, 2)
        _within(f2, ref, cc.errors(run(dtype=np.float32), ref), f"member 2 of 3 with a mask sum of 0.75, order {order}")
        assert all(f2[key].any() for key in f2 if key.startswith("grad"))


# ---- 5. launches -------------------------------------------------------------------------------------------------------------
def test_the_two_launches_make_the_step():
    case, k, P = cc.CASES[4], 2, 3
    n = case[0] + 3
    b = _Batch(case, [_member_problem(case, p) for p in range(P)], k, "on", n)
    for order in ORDERS:
        step = _run_pop(b, order)
        rows_only, both = _run_pop(b, order, launches=(pop_critic.ROWS_ONLY, pop_critic.APPLY_ONLY))
        # the rows launch writes q and the workspace only
        assert all(_same_bits(rows_only[kind][i][t], b.stacked[kind][i][t]) for kind in KINDS for i in range(k) for t in range(10))
        assert all((g == POISON).all() for net in rows_only["grad"] for g in net)
        assert _same_bits(rows_only["q"], step["q"])
        for key in step:
            if key == "q":
                assert _same_bits(both[key], step[key])
            else:
                assert all(_same_bits(x, y) for nx, ny in zip(both[key], step[key]) for x, y in zip(nx, ny)), key


# ---- 6. the learner on the self-actuated piano ---------------------------------------------------------------------------
def _state(pop):
    torch.cuda.synchronize()
    c = lambda group: [[t.detach().clone() for t in net] for net in group]
    return dict(p=c([pop._critic_tensors(net) for net in pop.critics]), target=c([pop._critic_tensors(net) for net in pop.targets]),
                m=c(pop._c_m), v=c(pop._c_v))


def _same_state(a, b):
    return [kind for kind in a for na, nb in zip(a[kind], b[kind]) for x, y in zip(na, nb) if not torch.equal(x, y)]


def _single_steps(pop, before, u, t):
    """`critic.step` per member on the population's own rows of range u from the state `before`, as Adam's step t."""
    P, B, n = pop.P, pop.B, pop.utd * pop.B
    lr = pop.critic_optimizer.param_groups[0]["lr"]
    step_size, bc2_sqrt = critic.adam_scalars(lr, t)
    out = {kind: [[torch.empty_like(x) for x in net] for net in before[kind]] for kind in before}
    nbytes = critic.workspace_bytes(pop.n_critics, pop.H1, pop.H2, B)
    ws = torch.zeros(max(nbytes // 4, 1), device=_dev())
    q = torch.zeros(pop.n_critics, P * n, device=_dev())
    for p in range(P):
        mine = {kind: [[x[p].clone() for x in net] for net in before[kind]] for kind in before}
        sets = lambda kind: [critic.set_entry(net) for net in mine[kind]]
        critic.step(pop._u_obs.data_ptr(), pop._u_action.data_ptr(), pop._u_y.data_ptr(), pop._u_mask.data_ptr(),
                    pop._mean_f32[p].data_ptr(), pop._inv_std_f32[p].data_ptr(), pop.obs_clip, sets("p"), sets("m"), sets("v"),
                    sets("target"), q.data_ptr(), ws.data_ptr(), nbytes, pop.D, pop.H1, pop.H2, pop.A, P * n, step_size, bc2_sqrt,
                    tau=pop.tau, threshold=pop._threshold, keep_scale=pop._keep_scale, ln_eps=pop.ln_eps, seed=pop.seed,
                    round_=pop._round, row_first=p * n + u * B, row_count=B, hip_stream=_stream())
        torch.cuda.synchronize()
        for kind in before:
            for net_o, net_m in zip(out[kind], mine[kind]):
                for o, m in zip(net_o, net_m):
                    o[p].copy_(m)
    return out, q


def test_fused_population_on_the_self_actuated_piano():
    E, P, C, B, utd, tau = 6, 3, 4, 16, 2, 0.25
    env_a, env_b = _piano_env(E), _piano_env(E)
    kw = dict(hidden=(32, 16), n_critics=2, capacity=C, batch_size=B, lr=1e-3, tau=tau, seed=21, utd=utd, dropout=0.5,
              gamma=[0.99, 0.9, 0.95], init_alpha=[1.0, 0.5, 0.2], critic_step="fused")
    a, b = population.DroQPopulation(env_a, P, **kw), population.DroQPopulation(env_b, P, **kw)
    a.collect(6); b.collect(6)
    # draw_and_act, target_range(u), critic_step(batch): critic.step per member on the population's own rows
    a.draw_and_act()
    for u in range(utd):
        batch = a.target_range(u)
        before = _state(a)
        loss = a.critic_step(batch)
        after = _state(a)
        assert a._c_t == u + 1 and tuple(loss.shape) == (P,) and bool(torch.isfinite(loss).all())
        want, q = _single_steps(a, before, u, u + 1)
        assert _same_state(after, want) == [], u
        assert all(not torch.equal(x, y) for kind in after for na, nb in zip(after[kind], before[kind]) for x, y in zip(na, nb))
        r = slice(u * B, (u + 1) * B)
        v = lambda t: t.view(P, utd * B)[:, r]
        assert torch.equal(a._u_q.view(2, P, utd * B)[:, :, r], q.view(2, P, utd * B)[:, :, r])
        assert torch.equal(loss, population.critic_losses([v(x) for x in a._u_q], v(a._u_y), v(a._u_mask)))
    # a foreign batch raises
    with pytest.raises(population.LearnError, match="range of the population's own minibatches"):
        a.critic_step({key: v.clone() for key, v in a.minibatch().items()})
    # update(1): finite statistics of length P, and every member's parameters change; the loss only on the last step
    b.load_state_dict(a.state_dict(include_replay=True))
    env_b.load_state_dict(env_a.state_dict())
    assert b._c_t == a._c_t and _same_state(_state(a), _state(b)) == []
    nets = [a.actor] + a.critics
    before = [t.detach().clone() for net in nets for t in net.parameters()] + [a.log_alpha.detach().clone()]
    asked, critic_step = [], a.critic_step
    a.critic_step = lambda batch, **kwargs: (asked.append(kwargs.get("loss", True)), critic_step(batch, **kwargs))[1]
    torch.manual_seed(9)
    stats_a = a.update(1)
    del a.critic_step
    torch.manual_seed(9)
    stats_b = b.update(1)
    torch.cuda.synchronize()
    assert asked == [False] * (utd - 1) + [True]
    assert set(stats_a) == {"critic_loss", "actor_loss", "alpha_loss", "alpha", "entropy", "masked"}
    assert all(v.shape == (P,) and np.isfinite(v).all() for v in stats_a.values()), stats_a
    after = [t.detach() for net in nets for t in net.parameters()] + [a.log_alpha.detach()]
    for x, y in zip(before, after):
        assert all(bool((x[p] != y[p]).any()) for p in range(P)) and bool(torch.isfinite(y).all())
    assert all(t.grad is None for c in a.critics for t in c.parameters())      # the actor pass's critic gradients are dropped
    assert not a.critic_optimizer.state                                          # torch's critic optimiser stays unused
    # two fused populations joined by a state_dict stay bit-identical through collect + update ...
    assert all(np.array_equal(stats_a[key], stats_b[key]) for key in stats_a)
    for _ in range(2):
        a.collect(2); b.collect(2)
        torch.manual_seed(4)
        stats_a = a.update(1)
        torch.manual_seed(4)
        stats_b = b.update(1)
        assert all(np.array_equal(stats_a[key], stats_b[key]) for key in stats_a)
    assert _same_state(_state(a), _state(b)) == [] and a._c_t == b._c_t
    assert all(torch.equal(x, y) for x, y in zip(a.actor.parameters(), b.actor.parameters()))
    # ... and a state_dict round trip continues with the same critic bits after one more critic_step
    b.load_state_dict(a.state_dict(include_replay=True))
    for pop in (a, b):
        pop.draw_and_act()
        pop.critic_step(pop.target_range(1))
    assert _same_state(_state(a), _state(b)) == [] and a._c_t == b._c_t
    # a cross-mode checkpoint raises, both ways
    plain = population.DroQPopulation(env_b, P, **dict(kw, critic_step="torch"))
    with pytest.raises(ValueError, match="written with critic_step = fused"):
        plain.load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="written with critic_step = torch"):
        b.load_state_dict(plain.state_dict())


# ---- 7. it learns --------------------------------------------------------------------------------------------------------
def test_fused_population_learns_a_toy_task_per_member():
    """test_gpu_population's toy task, hyper-parameters and criterion unchanged, plus critic_step="fused": the mean reward
    of every member's last 5 of 40 rounds is at least half-way from that of its first 5 to the optimum 0.  The torch
    mode's ratios (profiles/pop_gpu_tests.txt): 0.115 0.106 0.128 0.123."""
    torch.manual_seed(0)
    P = TOY["members"]
    env = _MemberToyEnv(TOY["n_envs"], seed=1, members=P)
    pop = population.DroQPopulation(env, P, critic_step="fused", **TOY["pop"])
    log = pop.train(TOY["rounds"], TOY["steps_per_round"], TOY["grad_steps"])
    curve = np.array([s["mean_reward"] for s in log])                   # [rounds, P]
    first5, last5 = curve[:5].mean(0), curve[-5:].mean(0)
    recorded = (0.115, 0.106, 0.128, 0.123)
    for p in range(P):
        print(f"toy task, fused critic step, member {p}: mean reward {first5[p]:.4f} (first 5 rounds) -> {last5[p]:.4f} (last 5); "
              f"ratio {last5[p] / first5[p]:.3f} (torch mode: {recorded[p]:.3f}); alpha {log[-1]['alpha'][p]:.4f}; "
              f"curve {[round(float(c), 3) for c in curve[::5, p]]}")
    assert (first5 < -0.1).all() and (last5 >= 0.5 * first5).all(), (first5, last5)
    assert all(np.isfinite(s["critic_loss"]).all() for s in log) and (log[-1]["episodes"] > 0).all()
