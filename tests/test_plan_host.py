"""Host tests of the planner (include/plan/rp_plan.h, robopianist_amd/planning.py): the twin's Philox against the paper's
known-answer vectors, the noise's moments, the twin's splines and shift, the binding's symbols and argument validation
(refused calls return before anything touches a device), and `state_views()` on the CPU test double."""

from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_reference as pr  # noqa: E402
from fake_physics import FakePhysics  # noqa: E402
from robopianist_amd import planning  # noqa: E402


# ---- the noise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", pr.KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    got = [int(w) for w in pr.philox4x32_10(counter, key)]
    assert got == list(want), " ".join(f"{w:08x}" for w in got)


def test_philox_is_elementwise():
    e, c = np.arange(7)[:, None], np.arange(5)[None, :]
    both = pr.philox4x32_10((3, e, c, 1), (11, 12))
    for i in (0, 6):
        for j in (0, 4):
            one = pr.philox4x32_10((3, i, j, 1), (11, 12))
            assert [int(w[i, j]) for w in both] == [int(w) for w in one]


def test_z_moments_over_1e5_draws():
    """Irwin-Hall of 12 uniforms: mean 0, variance 1, |z| <= 6.  Standard errors over 1e5 draws: 0.003 (mean) and 0.0045
    (variance), so the bounds are more than 6 sigma away."""
    zz = pr.z(1234, 5, 0, np.arange(1000)[:, None], np.arange(100)[None, :]).ravel()
    assert zz.size == 100_000
    print(f"z: mean {zz.mean():.5f} variance {zz.var():.5f} max |z| {np.abs(zz).max():.4f}")
    assert abs(zz.mean()) < 0.02
    assert 0.97 <= zz.var() <= 1.03
    assert np.abs(zz).max() <= 6.0
    # other rounds, rows and seeds are other draws
    assert not np.array_equal(zz[:100], pr.z(1234, 5, 1, np.arange(1), np.arange(100)).ravel())
    assert not np.array_equal(zz[:100], pr.z(1235, 5, 0, np.arange(1), np.arange(100)).ravel())
    assert not np.array_equal(zz[:100], zz[100:200])


def test_z_extremes_are_exact():
    """The integer definition at its ends: S = 0 -> -6, S = 12 (2^32 - 1) -> 6 - 12 * 2^-32."""
    lo = (np.int64(0) - (np.int64(6) << np.int64(32))).astype(np.float64) * 2.0 ** -32
    hi = (np.int64(12 * (2 ** 32 - 1)) - (np.int64(6) << np.int64(32))).astype(np.float64) * 2.0 ** -32
    assert lo == -6.0 and hi == 6.0 - 12 * 2.0 ** -32


# ---- the twin's splines ------------------------------------------------------------------------------------------------
def test_twin_splines_and_shift():
    rng = np.random.default_rng(0)
    k = rng.normal(size=(2, 3, 4))
    # linear, H = 5, P = 3: knots at steps 0, 2, 4; the midpoints are means up to rounding
    assert [pr.knot_step(pr.LINEAR, p, 5, 3) for p in range(3)] == [0, 2, 4]
    for p, h in enumerate((0, 2)):
        assert np.array_equal(pr.spline_value(k, pr.LINEAR, h, 5, 3), k[:, p])
    assert np.allclose(pr.spline_value(k, pr.LINEAR, 4, 5, 3), k[:, 2], rtol=0, atol=1e-15)
    assert np.allclose(pr.spline_value(k, pr.LINEAR, 1, 5, 3), 0.5 * (k[:, 0] + k[:, 1]), rtol=0, atol=1e-15)
    # zero-order, H = 5, P = 2: knot 0 for steps 0-2, knot 1 for 3-4; knot 1 sits at step 3
    assert [min(h * 2 // 5, 1) for h in range(5)] == [0, 0, 0, 1, 1]
    assert [pr.knot_step(pr.ZERO, p, 5, 2) for p in range(2)] == [0, 3]
    k2 = k[:, :2]
    assert np.array_equal(pr.spline_value(k2, pr.ZERO, 2, 5, 2), k2[:, 0])
    assert np.array_equal(pr.spline_value(k2, pr.ZERO, 3, 5, 2), k2[:, 1])
    # the shifted plan at step h is the old plan at step h + 1, on the knots
    s = pr.shift(k, pr.LINEAR, 5)
    for p in range(3):
        assert np.array_equal(s[:, p], pr.spline_value(k, pr.LINEAR, min(2 * p + 1, 4), 5, 3))
    s0 = pr.shift(k2, pr.ZERO, 5)
    assert np.array_equal(s0[:, 0], k2[:, 0]) and np.array_equal(s0[:, 1], k2[:, 1])
    assert np.array_equal(pr.shift(k[:, :1], pr.LINEAR, 5), k[:, :1])
    # a constant plan stays what it is under both
    c = np.broadcast_to(rng.normal(size=(2, 1, 4)), (2, 3, 4)).copy()
    assert np.array_equal(pr.shift(c, pr.LINEAR, 5), c) and np.array_equal(pr.shift(c, pr.ZERO, 5), c)


def test_twin_accumulate_and_select():
    ret, alive = np.zeros(3), np.ones(3, np.uint8)
    seq = [(pr.STEP_MID, 1.0), (pr.STEP_LAST, 2.0), (pr.STEP_FIRST, 0.0), (pr.STEP_MID, 4.0)]
    for h, (st, r) in enumerate(seq):
        reward = np.array([r, r, np.nan if h == 0 else r])
        pr.accumulate(ret, alive, reward, np.array([st, pr.STEP_MID, pr.STEP_MID], np.int32), 0.5 ** h)
    assert ret[0] == 1.0 + 0.5 * 2.0 and alive[0] == 0            # the LAST step counts, nothing after it
    assert ret[1] == 1.0 + 1.0 + 0.0 + 0.5 and alive[1] == 1
    assert np.isnan(ret[2])
    best, val, nom = pr.select(np.array([1.0, 3.0, 3.0, np.nan, np.nan, np.nan, -np.inf, np.nan, -np.inf]),
                               np.arange(9.0).reshape(9, 1, 1), 3)
    assert best.tolist() == [1, 0, 0] and val[0] == 3.0 and np.isnan(val[1]) and val[2] == -np.inf
    assert nom.ravel().tolist() == [1.0, 3.0, 6.0]


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_and_dims():
    L = planning.load_library()
    assert set(planning.EXPORTED_SYMBOLS) == {"rp_plan_fork", "rp_plan_sample", "rp_plan_action", "rp_plan_accumulate",
                                              "rp_plan_select", "rp_plan_shift", "rp_plan_dim", "rp_plan_last_error"}
    assert [getattr(L, s) for s in planning.EXPORTED_SYMBOLS]
    assert planning.dim("max_fields") == planning.MAX_FIELDS == 64
    assert planning.dim("wave_size") == 64
    assert planning.dim("nothing") == -1


_A = 0x1000   # a non-null address: a refused call never reads it


def _refused(entry, match, **values):
    args = planning.make_args(entry, **values)
    assert planning.call_raw(entry, args) != 0
    assert match in planning.last_error(), planning.last_error()


def test_argument_validation_refuses_before_any_launch():
    tab = planning.field_table([(_A, _A, 8)])
    fork = dict(fields=tab, n_fields=1, G=2, K=3, env_first=0, env_count=6)
    _refused("fork", "fields is NULL", **dict(fork, fields=None))
    _refused("fork", "K must be >= 1", **dict(fork, K=0))
    _refused("fork", "G must be >= 1", **dict(fork, G=0))
    _refused("fork", "outside the batch", **dict(fork, env_first=4, env_count=3))
    _refused("fork", "outside the batch", **dict(fork, env_first=-1))
    _refused("fork", "n_fields", **dict(fork, n_fields=65))
    _refused("fork", "n_fields", **dict(fork, n_fields=0))
    _refused("fork", "NULL pointer", fields=planning.field_table([(_A, None, 8)]), n_fields=1, G=2, K=3, env_count=6)
    _refused("fork", "row_bytes", fields=planning.field_table([(_A, _A, 0)]), n_fields=1, G=2, K=3, env_count=6)
    with pytest.raises(planning.PlanError, match="fields per launch"):
        planning.field_table([(_A, _A, 8)] * 65)
    a = planning.make_args("fork", **fork)
    a.struct_size -= 8
    assert planning.call_raw("fork", a) != 0 and "struct_size" in planning.last_error()

    sample = dict(nominal=_A, sigma=_A, lo=_A, hi=_A, knots=_A, G=2, K=3, P=3, nu=4, env_count=6)
    for name in ("nominal", "sigma", "lo", "hi", "knots"):
        _refused("sample", "NULL", **dict(sample, **{name: None}))
    _refused("sample", "K must be >= 1", **dict(sample, K=0))
    _refused("sample", "P must be >= 1", **dict(sample, P=0))
    _refused("sample", "outside the batch", **dict(sample, env_first=1))

    action = dict(knots=_A, out=_A, precision=64, spline=1, h=0, H=5, P=3, nu=4, n_rows=6, row_count=6)
    _refused("action", "NULL", **dict(action, out=None))
    _refused("action", "P must be >= 1", **dict(action, P=0))
    _refused("action", "(H - 1) % (P - 1)", **dict(action, H=6))
    _refused("action", "(H - 1) % (P - 1)", **dict(action, H=2, P=3))
    _refused("action", "h must lie", **dict(action, h=5))
    _refused("action", "precision", **dict(action, precision=16))
    _refused("action", "outside the batch", **dict(action, row_first=1))
    _refused("action", "spline must be", **dict(action, spline=2))

    acc = dict(ret=_A, alive=_A, reward=_A, step_type=_A, precision=64, weight=1.0, E=6, env_count=6)
    for name in ("ret", "alive", "reward", "step_type"):
        _refused("accumulate", "NULL", **dict(acc, **{name: None}))
    _refused("accumulate", "outside the batch", **dict(acc, env_first=6, env_count=1))

    sel = dict(ret=_A, knots=_A, nominal=_A, best_k=_A, best_return=_A, G=2, K=3, P=3, nu=4, group_count=2)
    for name in ("ret", "knots", "nominal", "best_k", "best_return"):
        _refused("select", "NULL", **dict(sel, **{name: None}))
    _refused("select", "K must be >= 1", **dict(sel, K=0))
    _refused("select", "outside the batch", **dict(sel, group_count=3))

    sh = dict(nominal=_A, spline=1, H=5, P=3, nu=4, G=2, group_count=2)
    _refused("shift", "NULL", **dict(sh, nominal=None))
    _refused("shift", "(H - 1) % (P - 1)", **dict(sh, H=4))
    _refused("shift", "P must be >= 1", **dict(sh, P=0))
    _refused("shift", "outside the batch", **dict(sh, group_first=2, group_count=1))
    # an empty range is accepted and launches nothing
    assert planning.call_raw("shift", planning.make_args("shift", **dict(sh, group_count=0))) == 0
    assert planning.call_raw("fork", planning.make_args("fork", **dict(fork, env_count=0))) == 0
    with pytest.raises(TypeError):
        planning.make_args("shift", nothing=1)


def test_check_plan_shape():
    assert planning.check_plan_shape("linear", 5, 3) == 1 and planning.check_plan_shape("zero", 5, 2) == 0
    assert planning.check_plan_shape("linear", 1, 1) == 1
    for bad in (("cubic", 5, 3), ("linear", 6, 3), ("linear", 2, 3), ("zero", 0, 1), ("zero", 3, 0)):
        with pytest.raises(ValueError):
            planning.check_plan_shape(*bad)


# ---- state_views on the CPU double ---------------------------------------------------------------------------------
class _ViewPhysics(FakePhysics):
    """FakePhysics with the live counterpart of its own state_dict."""

    def state_views(self):
        return {"qpos": self.qpos, "qvel": self.qvel, "ctrl": self._ctrl, "time": self.time}


def _flat(sd, prefix=""):
    out = {}
    for k, v in sd.items():
        if isinstance(v, dict):
            out.update(_flat(v, prefix + k + "."))
        else:
            out[prefix + k] = v
    return out


def _env(n_envs=3, **task_kwargs):
    import test_tasks_host as tth
    from robopianist_amd.suite import environment
    from robopianist_amd.suite.tasks import piano_with_shadow_hands
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        task = piano_with_shadow_hands.PianoWithShadowHands(midi=tth._get_test_midi(dt=0.01), control_timestep=0.01,
                                                            **dict(dict(n_steps_lookahead=2), **task_kwargs))
    return environment.Environment(task, n_envs=n_envs, physics=_ViewPhysics(task.scene, n_envs))


def test_state_views_have_state_dicts_keys_and_share_storage():
    env = _env()
    env.reset()
    env.step(torch.zeros((3, 45), dtype=torch.float64))
    views, sd = env.state_views(), _flat(env.state_dict())
    assert set(views) == set(sd) - {"random_state"}
    assert "needs_reset" in views and "physics.qpos" in views and "task._t_idx" in views and "task.piano._state" in views
    for name, v in views.items():
        assert isinstance(v, torch.Tensor) and v.shape[0] == 3, name
        assert v.dtype == sd[name].dtype and v.shape == sd[name].shape and torch.equal(v, sd[name]), name
        assert v.data_ptr() != sd[name].data_ptr(), name            # state_dict clones, state_views does not
    task = env.task
    assert views["task._t_idx"].data_ptr() == task._t_idx.data_ptr()
    assert views["task.piano._activation"].data_ptr() == task.piano._activation.data_ptr()
    assert views["physics.qpos"].data_ptr() == env.physics.qpos.data_ptr()
    assert views["needs_reset"].data_ptr() == env.needs_reset.data_ptr() and env.needs_reset.dtype == torch.bool
    # live: a write through the view is a write of the state
    views["task._t_idx"].fill_(2)
    assert task._t_idx.tolist() == [2, 2, 2]
    # and the pairing the planner's constructor makes of two such environments
    big = _env(n_envs=6)
    big.reset()
    fields = planning.match_state_views(views, big.state_views(), 3, 6)
    assert [f[0] for f in fields] == list(views)
    assert dict((f[0], f[3]) for f in fields)["task.piano._activation"] == 88    # bool [E, 88]: one byte each
    with pytest.raises(ValueError, match="share memory"):
        planning.match_state_views(views, views, 3, 3)
    with pytest.raises(ValueError, match="state differs"):
        planning.match_state_views({k: v for k, v in views.items() if k != "needs_reset"}, big.state_views(), 3, 6)
    other = _env(n_envs=6)
    other.task._goal_state = other.task._goal_state[:, :2].contiguous()
    with pytest.raises(ValueError, match="_goal_state"):
        planning.match_state_views(views, other.state_views(), 3, 6)


def test_state_views_refuses_episode_state_that_is_not_per_env_tensors():
    from robopianist_amd.suite import variations
    env = _env(randomize_hand_positions=True)
    with pytest.raises(ValueError, match="randomize_hand_positions"):
        env.state_views()
    aug = _env(augmentations=[variations.MidiTemporalStretch(prob=1.0, stretch_range=0.1)])
    with pytest.raises(ValueError, match="augmentations"):
        aug.state_views()


def test_state_views_of_the_self_actuated_piano():
    import test_tasks_host as tth
    from robopianist_amd.suite import environment
    from robopianist_amd.suite.tasks import self_actuated_piano
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        task = self_actuated_piano.SelfActuatedPiano(midi=tth._get_test_midi(dt=0.01), control_timestep=0.01)
    env = environment.Environment(task, n_envs=3, physics=_ViewPhysics(task.scene, 3))
    env.reset()
    views, sd = env.state_views(), _flat(env.state_dict())
    # (the one shared, constant bank slot is not per-env state)
    assert set(views) == set(sd) - {"random_state", "task._goal_bank", "task._len"}
    assert all(v.shape[0] == 3 for v in views.values())
    assert views["task._goal_state"].data_ptr() == task._goal_state.data_ptr()
