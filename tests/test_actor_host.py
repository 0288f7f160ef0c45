"""Host tests of the fused actor step (include/learn/rp_actor.h, robopianist_amd/actor.py): the float64 twin is torch's own
step (autograd on offpolicy.squashed_gaussian, actor_loss and alpha_loss, two torch.optim.Adam) with the twin's noise and
masks injected -- the independent check of the header's derivative formulae --, the step's counter words, the cases the
GPU tests run and the rule their seeds were chosen by, the binding's symbols, struct sizes and argument validation
(refused calls return before anything touches a device), and the learner's option.

Conditioning.  The GPU tests hold the kernels to 8 times the error of a float32 restatement; that is only fair where a
float32 restatement in another summation order lies close to the first one.  actor_cases.py states the rule; here it is
asserted for every case at its seed, and for the seeds below 60 also that no earlier seed passes (the two later ones,
4357 and 274, were found by the same actor_cases.first_seed; walking to them again would take most of a minute).
"""

from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import actor_cases as ac  # noqa: E402
import actor_reference as ar  # noqa: E402
import critic_reference as cr  # noqa: E402
import droq_reference as dr  # noqa: E402
from test_offpolicy_host import _SpecEnv  # noqa: E402
from robopianist_amd import actor, critic, droq, learning, population  # noqa: E402


# ---- the twin ------------------------------------------------------------------------------------------------------------
def _exact(lr_, t):
    """Adam's scalars of step t as torch computes them, in double."""
    return dict(step_size=lr_ / (1.0 - ac.BETAS[0] ** t), bc2_sqrt=np.sqrt(1.0 - ac.BETAS[1] ** t), eps=ac.EPS,
                omb1=1.0 - ac.BETAS[0], beta2=ac.BETAS[1], omb2=1.0 - ac.BETAS[1])


@pytest.mark.parametrize("case,mode,n", [(ac.FIRST_CASE, "on", 3), (ac.FIRST_CASE, "first", 3), (ac.CASES[4], "on", 4),
                                         (ac.CASES[3], "off", 3)], ids=str)
def test_float64_twin_is_torchs_step_with_the_noise_and_the_masks_injected(case, mode, n):
    p = ac.problem(case)
    t_actor, t_alpha = p.t[mode]
    raw = ar.step(**p.twin_kw(mode, n, actor_adam=_exact(ac.LR, t_actor), alpha_adam=_exact(ac.ALPHA_LR, t_alpha)),
                  dtype=np.float64)
    # the case has what the formulae branch on: the clamp's three kinds, masked rows, every critic selected
    lo, hi = ac.LOG_STD_BOUNDS
    assert (raw["head_l"] < lo).any() and (raw["head_l"] > hi).any() and raw["inside"].any() and not raw["inside"].all()
    assert np.array_equal(raw["inside"], (raw["head_l"] > lo) & (raw["head_l"] < hi))
    assert (p.kw["mask"] == 0).any() and (p.kw["mask"] == 1).any() and n >= 3
    assert set(raw["best"]) == set(range(n))
    assert np.array_equal(raw["q_min"], raw["q"].min(0)) and np.array_equal(raw["best"], raw["q"].argmin(0))
    if mode != "off":
        assert all(0 < k.sum() < k.size for pair in raw["masks"] for k in pair)
    want = ac.torch_step(p, mode, n, masks=None if mode == "off" else raw["masks"], noise=raw["noise"])
    got = ac.flat(raw)
    assert set(got) == set(want) == set(ac.keys())
    for k in ac.keys():
        bar = 1e-9 * max(float(np.abs(want[k]).max()), 1e-300)
        err = float(np.abs(got[k] - want[k]).max())
        assert got[k].shape == want[k].shape and err <= bar, (k, err, bar)
        if k.startswith("grad") or k == "log_alpha.grad":
            assert np.abs(got[k]).max() > 0


def test_the_first_critic_that_attains_the_minimum_is_selected():
    """Two copies of one critic, with dropout off, tie on every row: the earlier one is kept."""
    p = ac.problem(ac.CASES[1])
    kw = p.twin_kw("off", 2)
    kw["critics"] = [kw["critics"][1], kw["critics"][1]]
    raw = ar.step(**kw, dtype=np.float32)
    assert np.array_equal(raw["q"][0], raw["q"][1]) and not raw["best"].any()


# ---- the counters --------------------------------------------------------------------------------------------------------
def test_the_steps_counter_words_are_its_own():
    assert ar.NOISE_COUNTER == actor.NOISE_COUNTER == actor.dim("noise_counter") == 64
    assert ar.COUNTER == actor.COUNTER == actor.dim("counter") == 80
    words = list(range(3)) + list(range(16, 20)) + [dr.COUNTER + k for k in range(8)] + [cr.COUNTER + k for k in range(8)] + \
        [ar.NOISE_COUNTER + j for j in range(3)] + [ar.COUNTER + k for k in range(8)]
    assert len(set(words)) == len(words) == 34
    # the same (seed, round, row): another draw than the policy's, other masks than the targets' and the critic step's
    import learn_reference as lr
    rows, t = np.arange(64), dr.drop_threshold(0.5)
    mine, policy = ar.noise(ac.SEED, 3, rows, 8), lr.noise(ac.SEED, 3, rows, 8)
    assert mine.shape == policy.shape and (mine != policy).all() and abs(np.corrcoef(mine.ravel(), policy.ravel())[0, 1]) < 0.2
    assert abs(mine.mean()) < 0.2 and 0.8 < mine.std() < 1.2
    for i in range(4):
        for L in range(2):
            m = ar.masks(rows, 64, i, L, ac.SEED, 1, t)
            assert 0.4 < (m != dr.masks(rows, 64, i, L, ac.SEED, 1, t)).mean() < 0.6
            assert 0.4 < (m != cr.masks(rows, 64, i, L, ac.SEED, 1, t)).mean() < 0.6
    # the range a row is computed in changes neither its noise nor its masks
    assert np.array_equal(ar.noise(3, 2, np.arange(7, 19), 5), ar.noise(3, 2, rows, 5)[7:19])
    assert np.array_equal(ar.masks(np.arange(7, 19), 32, 1, 1, 3, 2, t), ar.masks(rows, 32, 1, 1, 3, 2, t)[7:19])


# ---- the cases and their seeds -------------------------------------------------------------------------------------------
def test_the_cases_are_the_issues():
    assert ac.CASES == [(5, 1, 16, 16, 1, .5), (17, 63, 48, 16, 45, .5), (33, 255, 256, 256, 45, .01), (35, 300, 64, 64, 128, .25),
                        (70, 20, 32, 32, 6, .25)]
    import droq_cases as dc
    assert ac.WIDE_CASES == dc.WIDE_CASES and len(ac.ALL_CASES) == 9 and set(ac.SEEDS) == set(ac.ALL_CASES)
    assert 2 * ac.CASES[1][4] == 90 and 90 % 16 and 2 * ac.CASES[3][4] == actor.dim("max_actions") * 2 == 256
    assert ac.CASES[4][0] > 2 * actor.dim("stage_rows") and ac.CASES[4][0] % actor.dim("tile_rows") == 6


@pytest.mark.parametrize("case", ac.ALL_CASES, ids=ac.case_id)
def test_gpu_cases_are_well_conditioned_and_show_what_they_are_for(case):
    p = ac.problem(case)
    rows = case[0]
    assert np.array_equal(p.kw["mask"], (np.arange(rows) % 4 != 2).astype(np.float32))
    assert ("first" in ac.modes(case)) == (case == ac.FIRST_CASE)
    lo, hi = ac.LOG_STD_BOUNDS
    for mode in ac.modes(case):
        for n in ac.n_critics(case):
            raw = p.ref_raw(mode, n)
            l = raw["head_l"]
            assert (l < lo).any() and (l > hi).any() and raw["inside"].any(), (mode, n)
            if rows >= 17:
                assert set(raw["best"]) == set(range(n)), (mode, n, np.bincount(raw["best"]))
            e32 = p.err32(mode, n)
            assert set(e32) == set(ac.keys())
            for which in (1, 2):
                for k, ep in p.err_perm(mode, n, which).items():
                    assert ep <= 4 * e32[k], (case, mode, n, k, ep, e32[k])
            assert all(np.abs(v).max() > 0 for k, v in p.ref(mode, n).items() if "grad" in k)
    # roughly thirds: a bias falls below, inside and above the clamp with probability 1/4, 1/2, 1/4, so among A >= 45 biases
    # a kind's share has a standard deviation of at most 0.065 and stays above 0.25 - 2.5 x 0.065 (with a few actions the
    # shares are those few draws')
    l = p.ref_raw("on", 1)["head_l"]
    if case[4] >= 45:
        assert min((l < lo).mean(), (l > hi).mean(), ((l > lo) & (l < hi)).mean()) > 0.0875
    assert ac.shows_what_it_is_for(p) == ""
    worst = ac.conditioning(p, stop=False)
    print(f"conditioning {case}: the permuted restatements' errors are at most {worst:.2f} x the first one's")
    assert worst <= 4
    # torch's own float32 step, the reference of the dropout-off GPU test, is as close to the float64 twin
    worst = ac.torch_conditioning(p)
    print(f"conditioning {case}: torch's float32 step on the CPU has at most {worst:.2f} x the restatement's error")
    assert worst <= 4
    assert not np.array_equal(p.ref("on", 1)["q_min"], p.ref("off", 1)["q_min"])      # the dropout of the case drops something


@pytest.mark.parametrize("case", [c for c in ac.ALL_CASES if ac.SEEDS[c] < 60], ids=ac.case_id)
def test_each_seed_is_the_first_that_passes(case):
    assert ac.first_seed(case, ac.SEEDS[case] + 1) == ac.SEEDS[case]
    ac.problem.cache_clear()


def test_the_later_seeds_pass_and_a_rejected_seed_is_rejected_for_a_reason():
    assert sorted(s for s in ac.SEEDS.values() if s >= 60) == [274, 4357]
    # seed 0 of the smallest case: rejected, and the rule says why
    p = ac.problem(ac.CASES[0], 0)
    assert ac.shows_what_it_is_for(p) != "" or ac.conditioning(p) > 4


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_dims_and_struct_sizes():
    L_ = actor.load_library()
    assert set(actor.EXPORTED_SYMBOLS) == {"rp_actor_step", "rp_actor_workspace", "rp_actor_dim", "rp_actor_last_error"}
    assert [getattr(L_, s) for s in actor.EXPORTED_SYMBOLS]
    assert actor.dim("max_critics") == actor.MAX_CRITICS == 4 and actor.dim("launches") == actor.LAUNCHES == 2
    assert actor.dim("max_hidden") == learning.MAX_HIDDEN == 256 and actor.dim("max_actions") == learning.MAX_ACTIONS
    assert actor.dim("tile_rows") == 16 and actor.dim("stage_rows") == 32 and actor.dim("stats") == len(actor.STATS) == 5
    assert actor.dim("nothing") == -1
    assert actor.PARAMS == ar.PARAMS and actor.STATS == ar.STATS
    assert (actor.STEP, actor.ROWS_ONLY, actor.APPLY_ONLY) == (0, 1, 2)
    # the layouts of the header on the LP64 ABI
    assert ctypes.sizeof(actor.Set) == 48 and ctypes.sizeof(actor.Adam) == 24 and ctypes.sizeof(actor.WorkspaceArgs) == 32
    assert ctypes.sizeof(actor.StepArgs) == 464
    a = actor.make_args("step")
    assert actor.call_raw("step", a) != 0 and "struct_size" not in actor.last_error()
    a.struct_size -= 8
    assert actor.call_raw("step", a) != 0 and "struct_size" in actor.last_error()
    w = actor.make_args("workspace", H1=16, H2=16, A=2, row_count=5)
    w.struct_size += 8
    assert actor.call_raw("workspace", w) != 0 and "struct_size" in actor.last_error()
    # each library keeps its own symbols
    assert not hasattr(critic.load_library(), "rp_actor_step") and not hasattr(L_, "rp_critic_step")


def test_workspace_size():
    # h1, ds1 [R][H1], h2, ds2 [R][H2], dout3 [R][2 A], the tiles' partial sums [T][H1 + H2 + 2 A + 4], rounded up to 16 bytes
    for H1, H2, A, R in ((16, 16, 1, 5), (256, 256, 45, 4096), (48, 16, 45, 17), (32, 32, 6, 70), (64, 64, 128, 35)):
        T = -(-R // 16)
        floats = R * (2 * H1 + 2 * H2 + 2 * A) + T * (H1 + H2 + 2 * A + 4)
        assert actor.workspace_bytes(H1, H2, A, R) == 4 * (-(-floats // 4) * 4)
    assert actor.workspace_bytes(16, 16, 3, 0) == 0
    for bad in (dict(H1=8), dict(H2=272), dict(A=0), dict(A=129), dict(row_count=-1)):
        with pytest.raises(actor.LearnError, match="rp_actor_workspace"):
            actor.workspace_bytes(**dict(dict(H1=16, H2=16, A=2, row_count=4), **bad))


_A = 0x1000   # a non-null address: a refused call never reads it


def _refused(match, **values):
    args = actor.make_args("step", **values)
    assert actor.call_raw("step", args) != 0
    assert match in actor.last_error(), actor.last_error()


class _Fake:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def _set(hole=None):
    return actor.set_entry([None if k == hole else _Fake(_A) for k in range(6)])


def _critic_set(hole=None):
    return critic.set_entry([None if k == hole else _Fake(_A) for k in range(10)])


def test_argument_validation_refuses_before_any_launch():
    tab = critic.set_table([_critic_set(), _critic_set()])
    need = actor.workspace_bytes(16, 32, 2, 4)
    adam = actor.adam_entry(1e-3, 2)
    sa = dict(obs=_A, mask=_A, mean=_A, inv_std=_A, obs_clip=5.0, p=_set(), m=_set(), v=_set(), grad=_set(), critics=tab,
              n_critics=2, log_alpha=_A, log_alpha_m=_A, log_alpha_v=_A, log_alpha_grad=_A, target_entropy=-2.0,
              log_std_min=-5.0, log_std_max=2.0, workspace=_A, workspace_bytes=need, drop_threshold=7, keep_scale=1.0,
              ln_eps=1e-5, actor_adam=adam, alpha_adam=adam, action=_A, logp=_A, q_min=_A, stats=_A, D=3, H1=16, H2=32, A=2,
              B=4, row_first=0, row_count=4)
    for name in ("obs", "mask", "mean", "inv_std"):
        _refused("a pointer is NULL", **dict(sa, **{name: None}))
    _refused("critics is NULL", **dict(sa, critics=None))
    _refused("log_alpha is NULL", **dict(sa, log_alpha=None))
    _refused("m and v of log_alpha must not be NULL", **dict(sa, log_alpha_m=None))
    _refused("m and v of log_alpha must not be NULL", **dict(sa, log_alpha_v=None))
    _refused("stats is NULL", **dict(sa, stats=None))
    for n in (0, 5):
        _refused("n_critics", **dict(sa, n_critics=n))
    _refused("obs_clip", **dict(sa, obs_clip=-1.0))
    _refused("log_std_min must be <= log_std_max", **dict(sa, log_std_min=2.5))
    _refused("log_std_min must be <= log_std_max", **dict(sa, log_std_max=float("nan")))
    for bad in (0.0, -1.0, float("nan")):
        _refused("keep_scale must be > 0", **dict(sa, keep_scale=bad))
        _refused("ln_eps must be > 0", **dict(sa, ln_eps=bad))
        for field, what in (("actor_adam", "the actor's optimiser"), ("alpha_adam", "the temperature's optimiser")):
            for name in ("step_size", "bc2_sqrt", "eps"):
                broken = actor.adam_entry(1e-3, 2)
                setattr(broken, name, bad)
                _refused(f"{name} of {what} must be > 0", **dict(sa, **{field: broken}))
    _refused("D must be", **dict(sa, D=0))
    for h in (0, 8, 24, 272):
        _refused("H1 must be", **dict(sa, H1=h))
        _refused("H2 must be", **dict(sa, H2=h))
    for A in (0, 129):
        _refused("A must be", **dict(sa, A=A))
    for k in range(6):
        _refused("the actor has a NULL", **dict(sa, p=_set(k)))
        _refused("the m of the actor has a NULL", **dict(sa, m=_set(k)))
        _refused("the v of the actor has a NULL", **dict(sa, v=_set(k)))
    for k in range(10):
        _refused("the critic 1 has a NULL", **dict(sa, critics=critic.set_table([_critic_set(), _critic_set(k)])))
    _refused("workspace is NULL", **dict(sa, workspace=None))
    _refused("is smaller than", **dict(sa, workspace_bytes=need - 1))
    _refused("is smaller than", **dict(sa, workspace_bytes=0))
    _refused("16-byte aligned", **dict(sa, workspace=_A + 4))
    for bad in (-1, 3):
        _refused("launches must be", **dict(sa, launches=bad))
    _refused("B must be", **dict(sa, B=0, row_count=0))
    _refused("outside the batch", **dict(sa, row_first=1, row_count=4))
    _refused("outside the batch", **dict(sa, row_first=-1))
    assert actor.last_error().startswith("rp_actor_step: ")
    # accepted: a zero-row range (nothing is launched; its workspace is empty), with or without the optional pointers
    assert actor.call_raw("step", actor.make_args("step", **dict(sa, row_count=0, workspace_bytes=0))) == 0
    bare = dict(sa, row_first=4, row_count=0, grad=actor.set_entry(), log_alpha_grad=None, action=None, logp=None, q_min=None)
    assert actor.call_raw("step", actor.make_args("step", **bare)) == 0
    assert actor.call_raw("step", actor.make_args("step", **dict(sa, row_count=0, log_std_min=2.0))) == 0
    with pytest.raises(actor.LearnError):
        actor.set_entry([_Fake(_A)] * 5)
    with pytest.raises(TypeError):
        actor.make_args("step", nothing=1)


def test_adam_entry_carries_torchs_doubles_as_floats():
    for t in (1, 3, 1000):
        e = actor.adam_entry(3e-4, t, eps=1e-6)
        step_size, bc2 = critic.adam_scalars(3e-4, t)
        assert (e.step_size, e.bc2_sqrt, e.eps) == (np.float32(step_size), np.float32(bc2), np.float32(1e-6))
        assert (e.one_minus_beta1, e.beta2, e.one_minus_beta2) == (np.float32(1 - 0.9), np.float32(0.999), np.float32(1 - 0.999))


# ---- the learner's option ------------------------------------------------------------------------------------------------
def _droq(**kw):
    args = dict(hidden=(16, 32), n_critics=3, capacity=4, batch_size=32, lr=1e-2, tau=0.25, seed=5, dropout=0.25, utd=3)
    args.update(kw)
    return droq.DroQ(_SpecEnv(4, (4, 3), 3), **args)


def test_the_option_its_state_and_the_cross_mode_checkpoint():
    for bad in ("other", "", None, "Fused"):
        with pytest.raises(ValueError, match="actor_step must be"):
            _droq(actor_step=bad)
    # the four combinations
    made = {(c, a): _droq(critic_step=c, actor_step=a) for c in ("torch", "fused") for a in ("torch", "fused")}
    for (c, a), d in made.items():
        assert (d.critic_mode, d.actor_mode) == (c, a)
        assert hasattr(d, "_c_m") == (c == "fused") and hasattr(d, "_a_m") == (a == "fused")
        sd = d.state_dict()
        assert ("critic_step" in sd["droq"]) == ("critic_adam" in sd) == (c == "fused")
        assert ("actor_step" in sd["droq"]) == ("actor_adam" in sd) == (a == "fused")
    plain, fused = made["torch", "torch"], made["torch", "fused"]
    assert _droq().actor_mode == "torch"
    # the same seed draws the same networks in both modes
    assert all(torch.equal(x, y) for x, y in zip(plain.actor.parameters(), fused.actor.parameters()))
    # m, v per tensor in the order of the ABI, zero; the workspace sized for one range; five statistics
    assert [tuple(t.shape) for t in fused._a_m] == [(16, 7), (16,), (32, 16), (32,), (6, 32), (6,)]
    assert [tuple(t.shape) for t in fused._a_v] == [tuple(t.shape) for t in fused._a_m]
    assert all(not bool(t.any()) for t in fused._a_m + fused._a_v + [fused._la_m, fused._la_v])
    assert tuple(fused._la_m.shape) == tuple(fused._la_v.shape) == tuple(fused.log_alpha.shape) == (1,)
    assert fused._a_t == fused._la_t == 0
    assert fused._a_bytes == actor.workspace_bytes(16, 32, 3, 32) and fused._a_ws.numel() * 4 >= fused._a_bytes
    assert tuple(fused._a_stats.shape) == (5,)
    sd = fused.state_dict()
    assert sd["droq"]["actor_step"] == "fused" and sd["actor_adam"]["actor"]["t"] == 0 and sd["actor_adam"]["log_alpha"]["t"] == 0
    assert len(sd["actor_adam"]["actor"]["m"]) == len(sd["actor_adam"]["actor"]["v"]) == 6
    fused._a_m[3].fill_(2.0)
    fused._la_v.fill_(0.5)
    fused._a_t, fused._la_t = 7, 9
    sd = fused.state_dict()
    again = _droq(actor_step="fused", seed=9)
    again.load_state_dict(sd)
    assert (again._a_t, again._la_t) == (7, 9) and bool((again._a_m[3] == 2.0).all()) and not bool(again._a_m[2].any())
    assert float(again._la_v) == 0.5 and float(again._la_m) == 0.0
    fused._a_m[3].fill_(3.0)
    assert bool((sd["actor_adam"]["actor"]["m"][3] == 2.0).all())                 # a snapshot, not a view
    with pytest.raises(ValueError, match="written with actor_step = fused, this learner has actor_step = torch"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="written with actor_step = torch, this learner has actor_step = fused"):
        fused.load_state_dict(plain.state_dict())
    # the two options are refused independently
    with pytest.raises(ValueError, match="written with critic_step = fused"):
        fused.load_state_dict(made["fused", "fused"].state_dict())
    # a fused step is a step on a range of the learner's own minibatch
    with pytest.raises(droq.LearnError, match='actor_step="fused" steps on a range of the learner\'s own minibatch'):
        fused.actor_step({k: v.clone() for k, v in fused.minibatch().items()})
    assert fused._fused_range(fused.minibatch()) == 2
    # the statistics come from the device array, in the order of the ABI
    fused._a_stats.copy_(torch.tensor([1.0, 2.0, 3.0, 4.0, 0.25]))
    got = fused._host_stats({"critic_loss": torch.tensor(7.0), "actor_stats": fused._a_stats})
    assert got == {"critic_loss": 7.0, "actor_loss": 1.0, "alpha_loss": 2.0, "alpha": 3.0, "entropy": 4.0, "masked": 0.25}
    assert plain._host_stats({"alpha": torch.tensor(2.0)}) == {"alpha": 2.0}


def test_the_population_refuses_the_option():
    env = _SpecEnv(4, (4, 3), 3)
    kw = dict(hidden=(16, 32), n_critics=2, capacity=4, batch_size=8, utd=2)
    with pytest.raises(ValueError, match='DroQPopulation has no fused actor step yet'):
        population.DroQPopulation(env, 2, actor_step="fused", **kw)
    with pytest.raises(ValueError, match="actor_step must be"):
        population.DroQPopulation(env, 2, actor_step="other", **kw)
    assert population.DroQPopulation(env, 2, **kw).actor_mode == "torch"
