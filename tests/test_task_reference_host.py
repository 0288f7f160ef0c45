"""CPU tests of the float64 twin of the fused task kernels (tests/task_reference.py) and of the cases the GPU tests run
(tests/task_cases.py).

The twin is the definition only if it says what the task layer's torch hooks say.  On the real two-hand and one-hand
tasks, built on the physics test double, synthetic joint angles, site positions, actuator sensors, contact pairs and warn
words are written into the physics -- forearm hits and wrong presses among them -- and the twin's float64 `rewards` must
equal `task.reward_fn.compute` term by term, its `prestep` CanonicalSpecWrapper + before_step bit for bit, and its
`advance`, chained over a few dozen steps across episode ends, every TimeStep field, every persistent array of the task
and the piano and the reduction of MidiEvaluationWrapper's torch path (floats to 1e-12, everything discrete exactly).

The cases are well conditioned: every seed is the first from 0 that passes the permuted-restatement rule, no discrete
output sits near its switch, every OT env's optimum is unique by a margin, and every case shows what it is for.
"""

from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import task_cases as tc  # noqa: E402
import task_reference as tr  # noqa: E402
from fake_physics import FakePhysics  # noqa: E402
from robopianist_amd.music import midi_file  # noqa: E402
from robopianist_amd.music.sequence import NoteSequence  # noqa: E402
from robopianist_amd.suite import environment  # noqa: E402
from robopianist_amd.suite.tasks import PianoWithOneShadowHand, base, piano_with_shadow_hands  # noqa: E402
from robopianist_amd.wrappers.canonical import CanonicalSpecWrapper  # noqa: E402
from robopianist_amd.wrappers.evaluation import MidiEvaluationWrapper  # noqa: E402

DT = 0.05
E = 6
npy = lambda t: t.detach().cpu().numpy().copy()


def _midi(fingering=True):
    """Nine frames, notes of both hands on keys of both halves of the keyboard, two at once, a pedal that goes down and up."""
    seq = NoteSequence()
    notes = ((0.0, 0.15, 60, 1), (0.0, 0.1, 36, 7), (0.1, 0.3, 100, 4), (0.15, 0.25, 90, 0), (0.2, 0.4, 30, 9), (0.3, 0.4, 64, 2),
             (0.3, 0.4, 66, 3))
    for s, e, p, part in notes:
        seq.notes.add(start_time=s, end_time=e, velocity=80, pitch=p, part=part if fingering else -1)
    seq.control_changes.add(time=0.1, control_number=64, control_value=100)
    seq.control_changes.add(time=0.3, control_number=64, control_value=10)
    seq.total_time = 0.4
    seq.tempos.add(qpm=60)
    return midi_file.MidiFile(seq=seq)


def _env(kind, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if kind in ("right", "left"):
            task = PianoWithOneShadowHand(midi=_midi(), hand_side=kind, control_timestep=DT, change_color_on_activation=True, **kw)
        else:
            task = piano_with_shadow_hands.PianoWithShadowHands(
                midi=_midi(), control_timestep=DT, change_color_on_activation=True, disable_fingering_reward=kind == "ot", **kw)
    return environment.Environment(task, n_envs=E, physics=FakePhysics(task.scene, E))


def _model_of(env, kind):
    """The kernels' "model constants" of a real task, as the task's own binding code hands them to the launch."""
    task = env.task
    hf = {"right": 1, "left": 2}.get(kind, 0)
    hands = [task._hand] if hf else [task.right_hand, task.left_hand]
    md = {"key_qadr": np.asarray(task.piano.joints, np.int64), "key_qrange": npy(task.piano._qpos_range),
          "key_anchor": npy(task._key_anchor), "key_half": npy(task._key_half),
          "hand_act": np.concatenate([np.asarray(h.actuators, np.int64) for h in hands]),
          "tip_site": np.asarray([int(s) for s in task._tip_sites], np.int64),
          "rfa": np.asarray([] if hf else task.right_hand.forearm_geom_ids, np.int64),
          "lfa": np.asarray([] if hf else task.left_hand.forearm_geom_ids, np.int64), "hand_filter": hf,
          "energy_coef": 5e-3, "key_close": 0.05, "finger_close": 0.01, "nv": env.physics.model.nv, "nu": env.physics.model.nu}
    uf = 2 if kind == "ot" else 1
    return md, tc.model_kw(md, uf, 0 if hf else 1)


def _write_physics(env, md, rng, pressed, on_keys, n):
    """Synthetic engine state into the test double: key angles with the given presses, fingertips near keys, actuator
    sensors, contact slots of every kind (forearm hits among them) and warn words."""
    phys = env.physics
    qk = np.stack([tc.key_angles(rng, md, pressed[e]) for e in range(E)])
    q = rng.uniform(-0.1, 0.1, (E, md["nv"]))
    q[:, md["key_qadr"]] = qk
    sites = rng.uniform(-1, 1, (E, phys._sites.shape[1], 3))
    for e in range(E):
        tgt = tc.key_targets64(md, q[e])
        for s in md["tip_site"]:
            k = on_keys[e][rng.integers(len(on_keys[e]))] if len(on_keys[e]) else rng.integers(88)
            v = rng.normal(size=3)
            sites[e, s] = tgt[k] + (0.004, 0.05, 0.2, 1.0)[rng.integers(4)] * v / np.linalg.norm(v)
    phys.qpos.copy_(torch.as_tensor(q))
    phys._sites.copy_(torch.as_tensor(sites))
    phys.act_force.copy_(torch.as_tensor(rng.normal(size=(E, md["nu"]))))
    phys.act_vel.copy_(torch.as_tensor(rng.normal(size=(E, md["nu"]))))
    if len(md["rfa"]):
        cg = np.stack([tc.contacts(rng, md, (e + n) % 8, 64) for e in range(E)])
        phys.contact_geoms.copy_(torch.as_tensor(cg))
    phys.warn.copy_(torch.as_tensor(np.asarray([(0, 0, 1, 0, 2, 64, 0)[(2 * e + n) % 7] for e in range(E)], np.int32)))


def _engine_views(env):
    p = env.physics
    return {"qpos": npy(p.qpos), "act_force": npy(p.act_force), "act_vel": npy(p.act_vel), "site_xpos": npy(p._sites),
            "contact_geoms": npy(p.contact_geoms), "warn": npy(p.warn)}


def _presses(rng, goal_rows, n):
    pressed = np.zeros((E, 88), bool)
    on_keys = []
    for e in range(E):
        keys = np.flatnonzero(goal_rows[e, :88] > 0)
        on_keys.append(keys)
        kind = (e + n) % 4
        if kind in (0, 2):
            pressed[e, keys] = True
        if kind == 2 and (n // 4) % 2:
            pressed[e, (87, 3, 64, 63)[(e + n) % 4]] = True       # a wrong press (unless the key is a goal)
        if kind == 3:
            pressed[e, keys[::2]] = True
    return pressed, on_keys


# ---- the twin is the definition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["two-hands", "ot", "right", "left"])
def test_twin_rewards_equal_the_tasks_reward_terms(kind):
    env = _env(kind)
    task = env.task
    md, mkw = _model_of(env, kind)
    env.reset()
    rng = np.random.default_rng(5)
    ntip = 5 if md["hand_filter"] else 10
    hit_seen, fp_seen = set(), set()
    for n in range(8):
        goal = np.zeros((E, 89))
        finger = np.full((E, 88), -1, np.int64)
        for e in range(E):
            keys = tc.goal_keys(rng, e + 6 * n)
            goal[e, keys] = 1.0
            finger[e, keys] = np.where(rng.random(len(keys)) < 0.2, -1, rng.integers(0, ntip, len(keys)))
        goal[:, 88] = rng.integers(0, 2, E)
        pressed, on_keys = _presses(rng, goal, n)
        _write_physics(env, md, rng, pressed, on_keys, n)
        task.after_substeps(env.physics)
        task._goal_current.copy_(torch.as_tensor(goal))
        task._finger_current.copy_(torch.as_tensor(finger))
        task.piano._sustain_activation.copy_(torch.as_tensor(rng.random((E, 1)) < 0.5))
        total = npy(task.reward_fn.compute(env.physics))
        assert np.array_equal(npy(task.piano.activation), pressed)
        got = tr.rewards(np.float64, **_engine_views_for_rewards(env), goal_current=goal, key_norm_state=npy(task.piano.normalized_state),
                         key_activation=pressed, sustain_activation=npy(task.piano.sustain_activation), finger_current=finger, **mkw)
        terms = task.reward_fn.reward_terms
        names = {"key_press": "key_press_reward", "sustain": "sustain_reward", "energy": "energy_reward",
                 "fingering": "ot_fingering_reward" if kind == "ot" else "fingering_reward", "forearm": "forearm_reward"}
        for i, name in enumerate(tr.TERMS):
            if names[name] in terms:
                np.testing.assert_allclose(got["terms"][i], npy(terms[names[name]]), rtol=0, atol=1e-12, err_msg=f"{name} round {n}")
            else:
                assert not got["terms"][i].any()
        np.testing.assert_allclose(got["total"], total, rtol=0, atol=1e-12)
        if "forearm_reward" in terms:
            hit_seen.update(npy(terms["forearm_reward"]).tolist())
        fp_seen.update((pressed & (goal[:, :88] == 0)).any(1).tolist())
    assert fp_seen == {False, True} and (kind in ("right", "left") or hit_seen == {0.0, 0.5})


def _engine_views_for_rewards(env):
    v = _engine_views(env)
    v.pop("warn")
    return v


def _task_state(env, ev):
    """Every persistent array the launch reads or writes, from the objects that own them on the torch path."""
    t, pn = env.task, env.task.piano
    return {"t_idx": npy(t._t_idx), "needs_reset": npy(env._needs_reset), "discount_state": npy(t._discount),
            "goal_state": npy(t._goal_state), "finger_next": npy(t._finger_next), "song_id": npy(t._song_id),
            "fatal_count": npy(t._fatal_count), "warn_count": npy(t._overflow_count), "key_state": npy(pn._state),
            "key_norm_state": npy(pn._normalized_state), "key_activation": npy(pn._activation),
            "sustain_activation": npy(pn._sustain_activation), "goal_current": npy(t._goal_current),
            "finger_current": npy(t._finger_current), "fingering_state": npy(t._fingering_state),
            "should_terminate": npy(t._should_terminate), "failure_termination": npy(t._failure_termination),
            "eval_sums": npy(ev._sums), "eval_count": npy(ev._count), "eval_hist": npy(ev._hist), "eval_nfinished": npy(ev._n_finished)}


@pytest.mark.parametrize("kind,options", [("two-hands", dict(wrong_press_termination=True, n_steps_lookahead=3)),
                                          ("two-hands", dict(overflow_termination=True, n_steps_lookahead=0)),
                                          ("ot", dict(n_steps_lookahead=12)),
                                          ("right", dict(wrong_press_termination=True, n_steps_lookahead=1)),
                                          ("left", dict(n_steps_lookahead=2))],
                         ids=["two-hands-wrong-press", "two-hands-overflow", "ot", "right", "left"])
def test_twin_prestep_and_advance_chain_equals_the_torch_hooks(kind, options):
    env = _env(kind, **options)
    can = CanonicalSpecWrapper(env, clip=True)
    deque = 3
    ev = MidiEvaluationWrapper(can, deque_size=deque)
    task, phys = env.task, env.physics
    md, mkw = _model_of(env, kind)
    spec = env.action_spec()
    lo, rng_ = spec.minimum.astype(np.float64), (torch.as_tensor(spec.maximum) - torch.as_tensor(spec.minimum)).numpy()
    ev.reset()
    rng = np.random.default_rng(17)
    const = {"goal_bank": npy(task._goal_bank), "finger_bank": npy(task._finger_bank), "song_len": npy(task._song_len),
             "key_qrange": md["key_qrange"]}
    adv = dict(n_lookahead=task._n_steps_lookahead, wrong_press_termination=int(task._wrong_press_termination),
               key_threshold=base._KEY_THRESHOLD, sustain_threshold=base._SUSTAIN_THRESHOLD, warn_fatal_mask=task.fatal_warn_mask,
               warn_count_mask=task.overflow_warn_mask, eval_deque=deque, **mkw)
    state = _task_state(env, ev)
    na = spec.shape[0]
    zeros = lambda *s: np.zeros(s)
    state.update(discount=zeros(E), step_type=np.zeros(E, np.int32), terms=zeros(5, E), total=zeros(E))
    types, fails = [], 0
    for n in range(40):
        pressed, on_keys = _presses(rng, state["goal_state"][:, 0], n)
        _write_physics(env, md, rng, pressed, on_keys, n)
        action = rng.uniform(-1.3, 1.3, (E, na))
        action[n % E, n % na] = (np.nan, np.inf, -np.inf)[n % 3]
        if n == 7:
            env.request_reset(torch.as_tensor(np.arange(E) == 2))
            state["needs_reset"] = npy(env._needs_reset)
        ctrl0 = npy(phys.ctrl)
        pre = tr.prestep(np.float64, action=action, needs_reset=state["needs_reset"], hand_act=md["hand_act"], ctrl=ctrl0,
                         sustain_state=npy(task.piano._sustain_state), act_lo=lo, act_range=rng_, clip=True)
        ts = ev.step(action)
        stepped = ~state["needs_reset"]
        # the pre-step: the action in the spec's units in ctrl (rows of the envs that are stepped) and the pedal's latch
        assert np.array_equal(npy(phys.ctrl)[stepped], pre["ctrl"][stepped], equal_nan=True)
        assert np.array_equal(npy(task.piano._sustain_state), pre["sustain_state"], equal_nan=True)
        assert np.array_equal(npy(phys.active), pre["active"].astype(bool)) and np.array_equal(pre["reset_mask"] != 0, state["needs_reset"])
        out = tr.advance(np.float64, {**state, **const, **_engine_views(env), "sustain_state": pre["sustain_state"]}, **adv)
        state = {**state, **out}
        now = _task_state(env, ev)
        now.update(step_type=npy(ts.step_type), total=npy(ts.reward), discount=npy(ts.discount))
        for k, v in now.items():
            if v.dtype.kind == "f":
                np.testing.assert_allclose(out[k], v, rtol=0, atol=1e-12, equal_nan=True, err_msg=f"{k} at step {n}")
            else:
                assert np.array_equal(out[k], v), (k, n)
        np.testing.assert_array_equal(npy(ts.observation["goal"]), out["goal_state"].reshape(E, -1))
        if "fingering" in ts.observation:
            np.testing.assert_array_equal(npy(ts.observation["fingering"]), out["fingering_state"])
        terms = task.reward_fn.reward_terms
        for i, name in enumerate(("key_press_reward", "sustain_reward", "energy_reward",
                                  "ot_fingering_reward" if kind == "ot" else "fingering_reward", "forearm_reward")):
            if name in terms:
                np.testing.assert_allclose(out["terms"][i], npy(terms[name]), rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
        types += out["step_type"].tolist()
        fails += int(out["failure_termination"].sum())
    assert set(types) == {0, 1, 2} and fails > 0 and state["eval_nfinished"].min() >= 2 * deque - 2
    assert state["fatal_count"].sum() > 0 and (kind != "two-hands" or state["warn_count"].sum() > 0)


def test_twin_scripted_index_equals_scripted_actions():
    from robopianist_amd.suite.scripted import ScriptedActions
    kw = tc.prestep_problem(tc.PRESTEP_CASES[2])
    table, idx = torch.as_tensor(kw["action_table"]), torch.as_tensor(kw["action_index"].copy())
    src = ScriptedActions(table, idx)
    taken = src.take().numpy()
    src.advance(torch.as_tensor(kw["needs_reset"]))
    plain = {k: v for k, v in kw.items() if k not in ("act_lo", "act_range", "clip")}
    out = tr.prestep(np.float64, **plain)
    assert np.array_equal(out["action_index"], idx.numpy()) and set(kw["action_index"].tolist()) == set(tc.TABLE_INDEX)
    stepped = ~kw["needs_reset"]
    assert np.array_equal(out["ctrl"][stepped][:, kw["hand_act"]], taken[stepped, :-1], equal_nan=True)
    assert (out["ctrl"][~stepped] == tc.POISON).all()


def test_twin_exact_edges_follow_the_contract():
    md, key, state, options, expect = tc.edge_problem()
    out = tr.advance(np.float64, state, **options)
    assert [bool(out["key_activation"][e, key[e]]) for e in range(5)] == expect["pressed"]
    assert out["sustain_activation"].ravel().tolist() == expect["sustain_on"]
    assert [out["key_state"][e, key[e]] for e in range(5)] == expect["key_state"]
    assert out["key_norm_state"][2, key[2]] == 1.0 and out["key_norm_state"][3, key[3]] == -0.5
    # env 1: goal 1, state 1 - key_close, nothing pressed: x == upper is inside the bounds, the term is exactly 1
    assert out["terms"][0, 1] == 1.0 and out["terms"][0, 0] == 1.0 and out["terms"][0, 2] == 1.0
    assert 0.5 < out["terms"][0, 3] < 0.5 + 1e-3


# ---- the cases are well conditioned -------------------------------------------------------------------------------------
ALL_REWARD = tc.REWARD_CASES + tc.OT_CASES


@pytest.mark.parametrize("case", ALL_REWARD, ids=tc.case_id)
def test_reward_case_seed_is_the_first_well_conditioned(case):
    assert tc.first_seed(tc.reward_problem, case) == tc.REWARD_SEEDS[case]
    p = tc.reward_problem(case)
    e32 = p.err32()
    # a float32 restatement that is exact has nothing to say: the terms that are sums of rounded numbers must have an error
    assert e32["forearm"] == 0.0 and (e32["energy"] > 0 and e32["total"] > 0)


@pytest.mark.parametrize("case", ALL_REWARD, ids=tc.case_id)
def test_reward_case_shows_what_it_is_for(case):
    E_, nv, hands, nc, (nr, nl), hf, uf, ufa = case
    p = tc.reward_problem(case)
    kw, md = p.kw, p.md
    assert kw["key_qadr"][0] != 0 and len(set(kw["key_qadr"].tolist())) == 88 and kw["key_qadr"].max() < nv
    assert len(kw["hand_act"]) == hands[1] and len(set(kw["hand_act"].tolist())) == hands[1] and kw["hand_act"].max() < hands[0]
    assert not hands[2] or (np.diff(kw["hand_act"]) < 0).any()
    assert kw["contact_geoms"].shape == (E_, nc, 2) and (len(kw["rfa"]), len(kw["lfa"])) == (nr, nl)
    hit = np.asarray([tc.hits(md, cg) for cg in kw["contact_geoms"]])
    ref = p.ref()
    if ufa:
        assert np.array_equal(ref["terms"][4] == 0.0, hit) and np.array_equal(ref["terms"][4] == 0.5, ~hit)
    if E_ == 70:
        kinds = np.asarray(p.contact_kinds) % 8
        assert hit[np.isin(kinds, (1, 2, 3, 7))].all() and not hit[np.isin(kinds, (0, 4, 5, 6))].any()
        assert (kw["contact_geoms"][kinds == 3][:, :nc - 1] < 0).all()       # a pair in the last slot only (69 of 70)
        sizes = {len(k) for k in p.on_keys}
        assert sizes == {0, 1, 4, 5, 6, 9, 10, 11, 88}
        assert {tuple(k) for k in p.on_keys if len(k) == 1} == {(0,), (63,), (64,), (87,)}
        # false positives whose only cause is a key of the second slot
        fp = kw["key_activation"] & (kw["goal_current"][:, :88] == 0)
        assert (fp[:, 64:].any(1) & ~fp[:, :64].any(1)).any() and (~fp.any(1)).any()
        # the tolerance's three regions among the goal keys: inside the bounds, on the flank, float32 exp underflows
        x = (kw["goal_current"][:, :88] - kw["key_norm_state"])[kw["goal_current"][:, :88] > 0]
        t32 = tr.tolerance(x, 0.05, 0.5, np.float32)
        assert (t32 == 1).any() and ((t32 > 0) & (t32 < 1)).any() and (t32 == 0).any() and (x < 0).any()
        on = kw["goal_current"][:, :88] > 0
        assert (kw["finger_current"][on] == -1).any() and (kw["finger_current"][on] >= 0).any()
    if uf == 2:
        assert all((a is None) == (len(k) == 0) for a, k in zip(ref["assignment"], p.on_keys))
        assert all(ref["terms"][3, e] == 1.0 for e, k in enumerate(p.on_keys) if len(k) == 0)


@pytest.mark.parametrize("case", [c for c in ALL_REWARD if c[6] == 2], ids=tc.case_id)
def test_ot_optimum_is_unique_by_a_margin(case):
    """Re-solve with each edge of the optimum forbidden in turn: the best alternative total must exceed the optimum by
    more than 1e-4, far above the float32 error of a distance and far below the spacing of the keys."""
    p = tc.reward_problem(case)
    margins = tc.ot_margins(p)
    assert all(gap > tc.OT_MARGIN for _, gap in margins), margins
    sizes = {n for n, _ in margins}
    ntip = 5 if case[5] else 10
    assert case[0] < 70 or {ntip - 1, ntip, ntip + 1, 88, 1} <= sizes


@pytest.mark.parametrize("name", list(tc.ADVANCE_CASES))
def test_advance_case_is_well_conditioned_and_shows_what_it_is_for(name):
    assert tc.first_advance_seed(name) == tc.ADVANCE_SEEDS[name]
    p = tc.advance_problem(name)
    c, E_ = p.c, p.E
    thr = tc.KEY_THRESHOLD
    lo, hi = p.md["key_qrange"][:, 0], p.md["key_qrange"][:, 1]
    types, words, ends = [], set(), []
    o32 = p.chain32()
    for n, (inp, ref) in enumerate(zip(p.launches, p.refs)):
        # no discrete output within rounding of its switch
        st = np.clip(inp["qpos"][:, p.md["key_qadr"]], lo, hi)
        assert (np.abs(np.abs(st - hi) - thr) >= 1e-4 * thr).all()
        assert (np.abs(inp["sustain_state"] - tc.SUSTAIN_THRESHOLD) >= 1e-4 * tc.SUSTAIN_THRESHOLD).all()
        # ... so the float32 restatement takes every decision the twin takes
        for k in p.written():
            if k not in p.float_keys() and k != "traj_record":
                assert np.array_equal(o32[n][k], ref[k]), (k, n)
        types += ref["step_type"].tolist()
        bits = np.flatnonzero(ref["key_activation"].any(0))
        words.update(bits.tolist())
        if p.low:
            assert (ref["goal_current"][:, :p.low] == 0).all() and not ref["key_activation"][:, :p.low].any()
            wrong = ref["key_activation"] & (ref["goal_current"][:, :88] == 0)
            assert not wrong[:, :87].any()
        ends.append(ref["step_type"] == 2)
    assert set(types) == {0, 1, 2}
    assert set(tc.BIT_KEYS) & words == {k for k in tc.BIT_KEYS if k >= p.low}
    last = p.refs[-1]
    if c["deque"]:
        assert (last["eval_nfinished"] - p.init["eval_nfinished"]).max() >= 2 * c["deque"]      # the ring wrapped twice
    if p.low:
        assert any(r["failure_termination"].any() for r in p.refs)
    if E_ >= 5:
        assert (last["fatal_count"] > p.init["fatal_count"]).any() and (last["warn_count"] > p.init["warn_count"]).any()
        # envs at the start, one before the end, at the end and past it; songs of 1, bank_len - 3 and bank_len rows
        assert set(p.const["song_len"].tolist()) == {1, tc.BANK_LEN - 3, tc.BANK_LEN}
        slen = p.const["song_len"][p.init["song_id"]]
        assert (p.init["t_idx"] == 0).any() and (p.init["t_idx"] == slen - 1).any() and (p.init["t_idx"] > slen).any()
        assert p.init["needs_reset"].any() and not p.init["needs_reset"].all()
    if c.get("prefetch"):
        seen = set()
        state = p.init
        for inp, ref in zip(p.launches, p.refs):
            ready = np.asarray(state["next_ready"]) | inp["ready_set"]
            seen.update(zip(ready.astype(bool).tolist(), np.asarray(state["needs_reset"]).tolist(), (np.asarray(state["song_id"]) % 2).tolist()))
            switched = ready.astype(bool) & np.asarray(state["needs_reset"])
            assert np.array_equal(ref["song_id"], np.asarray(state["song_id"]) ^ switched)
            state = ref
        assert len(seen) == 8, seen       # ready x resetting x the slot's parity


def test_prestep_and_raster_cases_show_what_they_are_for():
    assert {c[1] for c in tc.PRESTEP_CASES} == {1, 16, 17, 46} and {c[0] % 4 for c in tc.PRESTEP_CASES} == {1, 2}
    for case in tc.PRESTEP_CASES:
        kw = tc.prestep_problem(case)
        a = kw["action_table"] if kw["action"] is None else kw["action"]
        assert case[1] == 1 or (np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any() and (np.abs(a) > 1).any())
        out = tr.prestep(np.float32, **kw)
        untouched = np.ones_like(out["ctrl"], bool)
        untouched[np.ix_(~kw["needs_reset"], kw["hand_act"])] = False
        assert (out["ctrl"][untouched] == tc.POISON).all() and (case[2] == case[1] - 1 or untouched[~kw["needs_reset"]].any())
        if case[5]:
            assert np.nanmax(out["ctrl"][~untouched]) <= (kw["act_lo"] + kw["act_range"]).max() + 1e-6
    for case in tc.RASTER_CASES:
        out = tr.rasterize(np.float64, **tc.raster_kw(case))
        slots = [j[0] for j in tc.RASTER_JOBS]
        assert sorted(slots) != slots and out["status"].tolist() == [0, 0, 0, 1, 0, 0, 0]
        assert (out["goal_bank"][[2, 6]] == tc.POISON).all() and (out["song_len"][[2, 6]] == tc.IPOISON).all()
        nb = case[1]
        fr = lambda t: nb + int(t / case[0] + 1e-9)
        g, f = out["goal_bank"][4], out["finger_bank"][4]
        assert g[fr(0.30), 60 - 21] == 1 and g[fr(0.30) + 1, 60 - 21] == 0                       # the zero-length note
        assert g[fr(0.15), 64 - 21] == 1 and g[fr(0.20), 64 - 21] == 0 and g[fr(0.35), 64 - 21] == 1   # velocity 0 over a note
        assert g[fr(0.15), 67 - 21] == 1 and g[fr(0.20), 67 - 21] == 0 and g[fr(0.20) + 1, 67 - 21] == 1   # the repeated note
        assert f[fr(0.15), 67 - 21] == 8 and f[fr(0.20) + 1, 67 - 21] == 4
        back = out["goal_bank"][1]
        assert g[:, 87].any() and g[:, 86].any() and not back[:, 86:88].any() and back[:, 0].any()  # deleted notes stay deleted
        assert (g[:nb] == 0).all() and (f[:nb] == -1).all()
        twice = out["goal_bank"][0][:, 70 - 21]
        assert twice[fr(0.15)] == 1 and twice[fr(0.20)] == 0 and twice[fr(0.25)] == 0 and twice[fr(0.25) + 1] == 1   # two onsets in a row
        sus = out["goal_bank"][0][nb:, 88]
        assert sus[fr(0.10) - nb] == 1 and sus[fr(0.22) - nb] == 0 and sus[fr(0.40) - nb] == 1 and sus[fr(0.52) - nb] == 0
    assert len(tc.FULL_CHAIN) == 8
