"""The split position stage's own kernels (rp_pos_front_kernel / rp_pos_back_kernel) request the tables of a phase in one
batch -- clamped indices, unconditional reads, selects afterwards -- where the one-kernel stage reads every table where it
is used, under its predicate (csrc/rp_kernels.hpp: PF / PB).  Same operations on the same values: the split stage must
reproduce the one-kernel stage bit for bit.  The large-batch twins (3080 / 1100 envs) are
test_split_position_stage_is_bit_identical and test_stream_slices_and_cost_order_are_bit_identical; here: small batches,
the MESH = 2 kernel build (cylinder colliders), joint-limit rows through the now unconditional solimp read, and an env
whose candidate list is longer than one 64-lane chunk of the back part's collection loop.

No torch in here: the file also runs against the wave-emulator build (RP_ENGINE_LIB, tests/wavesim)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SCENES = {
    "hull": dict(primitive_fingertip_collisions=False),
    "capsule": dict(primitive_fingertip_collisions=True),
    "cylinder": dict(primitive_fingertip_collisions=False, cylinder_colliders=True),   # hull tips: the MESH = 2 build
}


def _scene(name):
    from robopianist_amd.model import scene
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return scene.build_scene(gravity_compensation=True, **_SCENES[name])


def _replay_ctrl(si):
    """The headline replay's controls, one row per control step (tests/test_gpu_parity.py: _replay_ctrl, every tenth row)."""
    m = si.model
    a = np.load("tests/golden/twinkle_twinkle_actions.npy").astype(np.float64)[:, :-1]
    lo, hi = m.actuator_ctrlrange[:, 0], m.actuator_ctrlrange[:, 1]
    return lo + (np.clip(a, -1, 1) + 1.0) * 0.5 * (hi - lo)


def _reference(si, E):
    from robopianist_amd import engine
    ref = engine.BatchedPhysics(si.model, si.key_joint_ids, n_envs=E, precision=64)
    ref.set_split_position_stage(False); ref.set_stream_slices(1); ref.set_fused_substeps(False); ref.set_acc_sensors(True)
    assert not ref.split_position_stage
    return ref


def _split(si, E, slices):
    from robopianist_amd import engine
    p = engine.BatchedPhysics(si.model, si.key_joint_ids, n_envs=E, precision=64)
    p.set_split_position_stage(True); p.set_stream_slices(slices); p.set_fused_substeps(False); p.set_acc_sensors(True)
    assert p.split_position_stage
    return p


def _assert_same(ref, p, tag):
    from robopianist_amd import engine
    assert np.array_equal(ref.qpos, p.qpos), tag
    assert np.array_equal(ref.qvel, p.qvel), tag
    for f in (engine.NCON, engine.CONTACT_GEOMS, engine.CONTACT_DIST, engine.SENSOR_TORQUE, engine.SENSOR_TOUCH):
        assert np.array_equal(ref.get(f), p.get(f)), (tag, f)


def _hand_dofs_beyond_range(si, qpos):
    """Hand dofs (every limited joint that is no key) outside their range, from the model's host-side joint ranges."""
    m = si.model
    hand = np.ones(m.nv, bool); hand[np.asarray(si.key_joint_ids)] = False
    hand &= np.asarray(m.jnt_limited).astype(bool)
    lo, hi = m.jnt_range[:, 0], m.jnt_range[:, 1]
    return int((((qpos < lo[None, :]) | (qpos > hi[None, :])) & hand[None, :]).sum())


def small_batch(scene_name, E=24, nsteps=30, nsub=10):
    """Returns (max contacts, hand dofs beyond their range summed over steps and envs); asserts the bits."""
    from robopianist_amd import engine
    si = _scene(scene_name)
    m = si.model
    ctrl = _replay_ctrl(si)
    rng = np.random.default_rng(2)
    gain = 1 + 0.1 * rng.standard_normal((E, 1))
    phase = rng.integers(0, 40, E)
    lo, hi = m.actuator_ctrlrange[:, 0], m.actuator_ctrlrange[:, 1]
    ref = _reference(si, E)
    modes = [_split(si, E, 1), _split(si, E, 3)]
    beyond, maxcon = 0, 0
    for t in range(nsteps):
        c = ctrl[(t + 20 + phase) % len(ctrl)] * gain
        c[3] = hi; c[E // 2 - 1] = lo; c[E - 5] = np.where(np.arange(m.nu) % 2 == 0, lo, hi)   # (held at the range ends: joint limits)
        for p in [ref] + modes:
            p.set(engine.CTRL, c)
            if t == nsteps // 4 + 1:
                mask = np.zeros(E, np.uint8); mask[::7] = 1
                p.reset(mask)
            if t == nsteps // 3 + 2:
                act = np.ones(E, np.int32); act[5] = 0
                p.set(engine.ACTIVE, act)
            if t == nsteps // 3 + 3:
                p.set(engine.ACTIVE, None)
            p.step(nsub)
        for i, p in enumerate(modes):
            _assert_same(ref, p, (t, i))
            assert p.warn_flags.max() == 0
        beyond += _hand_dofs_beyond_range(si, ref.qpos)
        maxcon = max(maxcon, int(ref.get(engine.NCON).max()))
    return maxcon, beyond


@pytest.mark.parametrize("scene_name", ["hull", "capsule", "cylinder"])
def test_small_batch_split_stage_is_bit_identical(scene_name):
    """24 envs (more than the 8 list stripes; three slices' worth of 8), the split stage forced with 1 and with 3 slices
    asked for (below 1024 envs the engine runs any request as one slice: the three-stream schedule itself is the 3080-env
    test's), 30 control steps of the replay with per-env phase and gain, one masked reset, one env sitting out a step.
    Three envs hold their controls at a ctrlrange end, which drives hand joints into their limits: the limit rows' solimp
    is an unconditional read in the back part now."""
    maxcon, beyond = small_batch(scene_name)
    print(f"{scene_name}: max contacts {maxcon}, hand dofs beyond their range (summed over steps and envs) {beyond}")
    assert maxcon >= 3, maxcon
    assert beyond >= 1, beyond


def long_candidate_list(E=16, nsteps=10, nsub=10):
    """Returns (candidates per position stage of env 0: the largest per-control-step mean, max contacts); asserts the bits.
    The count comes from a third engine (split stage, no sensor stage, same controls): slot 30 of the profile counters sums
    the candidates of env 0's position stages, nsub of them per control step -- divided by nsub + 1 here, so that a
    leading stage, if the engine ran one, could only lower the figure."""
    from robopianist_amd import engine
    si = _scene("capsule")
    m = si.model
    ref = _reference(si, E)
    p = _split(si, E, 1)
    cnt = engine.BatchedPhysics(m, si.key_joint_ids, n_envs=E, precision=64)
    cnt.set_split_position_stage(True); cnt.set_stream_slices(1); cnt.set_fused_substeps(False)
    ntree = ref.dim("ntree")
    rng = np.random.default_rng(5)
    off = np.zeros((E, ntree, 3))
    off[:, :, 2] = -rng.uniform(0.0965, 0.1045, (E, 1))
    off[0, :, 2] = -0.104
    lo, hi = m.actuator_ctrlrange[:, 0], m.actuator_ctrlrange[:, 1]
    c = lo + rng.uniform(0.3, 0.7, (E, m.nu)) * (hi - lo)
    for e in (ref, p, cnt):
        e.set(engine.TREE_OFFSET, off)
        e.set(engine.CTRL, c)
    cnt.profile(True)
    maxcon, best = 0, 0.0
    for t in range(nsteps):
        ref.step(nsub); p.step(nsub); cnt.step(nsub)
        _assert_same(ref, p, t)
        assert np.array_equal(ref.qpos, cnt.qpos), t
        maxcon = max(maxcon, int(ref.get(engine.NCON).max()))
        prof = cnt.profile(True)   # (reads and clears: this control step's counts)
        best = max(best, prof[30] / (nsub + 1))
    cnt.profile(False)
    return best, maxcon


def test_candidate_list_longer_than_one_chunk():
    """Both hands lowered until palms and fingers lie on the keys (rp_set(RP_TREE_OFFSET), as
    test_teacher_forced_fp64_palm_flat_on_the_keys lowers one): env 0's candidate list -- the profile counters' slots
    30: candidates narrow-phased in env 0's position stages, read per control step -- is longer than 64, the back part's
    collection loop takes a second, third and fourth chunk with the record requested ahead (on the wave emulator: 205 to
    248 candidates per stage over the first substeps, of a capacity of 256).  16 envs at different depths, 10 control
    steps; contact and key-slot capacities overflow in this pose, which both ways of running the stage must handle alike."""
    mean_cand, maxcon = long_candidate_list()
    print(f"env 0: at least {mean_cand:.1f} candidates per position stage (largest per-step mean); max contacts {maxcon}")
    assert mean_cand > 64, mean_cand   # (a mean above 64: at least one stage of that step took the second chunk)
    assert maxcon >= 3
