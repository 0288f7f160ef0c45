"""The reset snapshot (include/rp_engine.h: rp_set_reset_snapshot): a reset copies the position / velocity stage's results
for the reset state from a one-env shadow instead of the env going through the leading stage of the next rp_step.

Every test runs two engines on identical inputs, one with the switch ON and one with it OFF, and compares them bit for bit
after every control step.  The yardstick is the engine's own leading stage (switch off), never the snapshot path itself;
the step AFTER a reset is what proves the copied hand-over, since the solver stage of that step reads nothing else.

The comparison (`run_pair`) is shared with the CPU wave emulator: tests/wavesim/reset_snapshot.py runs it there without a
GPU (tests/test_wavesim_reset_snapshot.py)."""
import os
import warnings

import numpy as np
import pytest

from robopianist_amd import engine

NSUB = 10
FIELDS = ("QPOS", "QVEL", "QACC_WARMSTART", "NCON", "CONTACT_GEOMS", "CONTACT_DIST", "SITE_XPOS", "ACT_VELOCITY",
          "WARN_FLAGS", "SOLVER_ITER")
ON_EMULATOR = "wavesim" in os.environ.get("RP_ENGINE_LIB", "")

_scenes = {}


def hull_scene(primitive=False):
    from robopianist_amd.model import scene
    if primitive not in _scenes:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _scenes[primitive] = scene.build_scene(gravity_compensation=True, primitive_fingertip_collisions=primitive)
    return _scenes[primitive]


def replay_ctrl(si):
    """The Twinkle replay's rows as ctrl (one row per control step)."""
    m = si.model
    a = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twinkle_twinkle_actions.npy"))
    a = a.astype(np.float64)[:, :-1]
    lo, hi = m.actuator_ctrlrange[:, 0], m.actuator_ctrlrange[:, 1]
    return lo + (np.clip(a, -1, 1) + 1.0) * 0.5 * (hi - lo)


def ctrl_at(rows, t, E, first_row=24, stride=9):
    """Row of control step t for every env: env e is `stride * e` rows ahead, so that the envs differ and some touch keys."""
    return rows[(first_row + t + stride * np.arange(E)) % len(rows)]


class _Masks:
    """Reset masks as the engine wants them: device memory for rp_step_masked (a torch tensor on the GPU; on the
    emulator a numpy array while WAVESIM_DEVICE_PTRS=1 tells it to take host pointers for device ones)."""

    def __init__(self):
        self.keep = []

    def device(self, mask):
        mask = np.ascontiguousarray(mask, np.uint8)
        if ON_EMULATOR:
            self.keep.append(mask)
            return mask
        import torch
        t = torch.as_tensor(mask, device="cuda")
        torch.cuda.synchronize()   # (the engines run on streams of their own)
        self.keep.append(t)
        return t


def step_masked(p, masks, mask, nsub=NSUB):
    """rp_step_masked as the env layer calls it: the flagged envs are reset and sit the step out."""
    p.set(engine.ACTIVE, (1 - mask).astype(np.int32))
    dm = masks.device(mask)
    if ON_EMULATOR:
        os.environ["WAVESIM_DEVICE_PTRS"] = "1"
    try:
        p.step_masked(nsub, None, dm)
    finally:
        if ON_EMULATOR:
            os.environ["WAVESIM_DEVICE_PTRS"] = "0"
    p.sync()


def assert_equal_state(a, b, where):
    for f in FIELDS:
        x, y = a.get(getattr(engine, f)), b.get(getattr(engine, f))
        assert x.tobytes() == y.tobytes(), (where, f, np.argwhere(np.asarray(x != y))[:4].tolist())


def make_pair(si, E, precision=64, configure=None):
    """(switch on, switch off), both configured alike."""
    pair = []
    for on in (True, False):
        p = engine.BatchedPhysics(si.model, si.key_joint_ids, n_envs=E, precision=precision)
        p.set_reset_snapshot(on)
        if configure:
            configure(p)
        pair.append(p)
    return pair


def mask_plan(E, bounds=None):
    """control step -> reset mask (None: a plain rp_step; "contact": chosen at run time).  `bounds`: the slice bounds of
    the schedule under test (first env of every slice, then E), one slice by default."""
    bounds = bounds or [0, E]

    def m(*envs):
        x = np.zeros(E, np.uint8)
        x[list(envs)] = 1
        return x
    plan = {
        1: m(E // 2),                                   # one env alone
        2: m(bounds[0] + 1, bounds[-2] + 2),            # two envs (in different slices where there are slices)
        3: m(bounds[-2], bounds[-1] - 1),               # the first and the last env of a slice
        4: m(3), 5: m(3),                               # the same env on two consecutive steps
        6: np.ones(E, np.uint8),                        # all envs at once
        9: "contact",                                   # an env that is in contact and carries a warn bit
    }
    if len(bounds) > 2:
        plan[7] = m(bounds[1] - 1, bounds[1])           # both sides of a slice seam
    return plan


def run_pair(si, E, precision=64, configure=None, nsteps=12, bounds=None, between=None, plan=None, need_contact=True,
             nsub=NSUB):
    """Steps both engines through `nsteps` control steps with the reset masks of `plan`, comparing after every step.
    between(p, t, which): called for both engines in front of step t (fallback tests write state there)."""
    rows = replay_ctrl(si)
    a, b = make_pair(si, E, precision, configure)
    plan = mask_plan(E, bounds) if plan is None else plan
    masks = _Masks()
    seen_contact = 0
    reset_in_contact = False
    for t in range(nsteps):
        mask = plan.get(t)
        if isinstance(mask, str):
            ncon = b.get(engine.NCON)
            e = int(np.argmax(ncon))
            reset_in_contact = ncon[e] > 0
            mask = np.zeros(E, np.uint8)
            mask[e] = 1
            w = b.get(engine.WARN_FLAGS)
            w[e] |= engine.WARN_HESSIAN     # (a warn bit of the old episode: the reset clears it on both sides)
            for p in (a, b):
                p.set(engine.WARN_FLAGS, w)
        c = ctrl_at(rows, t, E)
        for i, p in enumerate((a, b)):
            p.set(engine.CTRL, c)
            if between:
                between(p, t, i)
            if mask is None:
                p.set(engine.ACTIVE, np.ones(E, np.int32))
                p.step(nsub)
            else:
                step_masked(p, masks, mask, nsub)
        assert_equal_state(a, b, ("step", t))
        seen_contact = max(seen_contact, int(b.get(engine.NCON).max()))
    print(f"reset snapshot on == off over {nsteps} control steps, {E} envs, fp{precision}; max contacts {seen_contact}; "
          f"reset an env in contact: {reset_in_contact}")
    if need_contact:
        assert seen_contact > 0
        if any(isinstance(v, str) and k < nsteps for k, v in plan.items()):
            assert reset_in_contact
    assert int(b.get(engine.WARN_FLAGS).max()) == 0
    return a, b


def one_kernel(p):
    p.set_stream_slices(1); p.set_split_position_stage(False); p.set_fused_substeps(False)


def split_stage(p):
    p.set_stream_slices(1); p.set_split_position_stage(True); p.set_fused_substeps(False)


def fused(p):
    p.set_stream_slices(1); p.set_fused_substeps(True)


def lazy(p):
    one_kernel(p); p.set_lazy_position_stage(True)


def lazy_split_ordered(p):
    split_stage(p); p.set_lazy_position_stage(True); p.set_cost_ordered_launch(True)


def slice_bounds(E, n):
    return [(E * s // n + 7) // 8 * 8 for s in range(n)] + [E]   # (rp_schedule.hpp: rp_slice_bound)


# ---------------------------------------------------------------------------------------------------- schedules
@pytest.mark.gpu
@pytest.mark.parametrize("schedule", [one_kernel, split_stage, fused, lazy, lazy_split_ordered],
                         ids=lambda f: f.__name__)
def test_snapshot_is_bit_identical_8_envs(schedule):
    run_pair(hull_scene(), 8, configure=schedule)


@pytest.mark.gpu
def test_snapshot_is_bit_identical_fp32():
    def conf(p):
        p.set_stream_slices(1); p.set_fused_substeps(False)
    run_pair(hull_scene(), 8, precision=32, configure=conf)


@pytest.mark.gpu
@pytest.mark.parametrize("slices", [2, 3])
@pytest.mark.parametrize("E", [24, 1032])
def test_snapshot_is_bit_identical_with_slices(E, slices):
    """24 envs with two / three slices asked for (the engine runs batches under 1024 envs as one slice, so that size shows
    the setter is harmless) and 1032 envs, where the slices are real: the split stage on every slice's own stream, lazy
    mode and cost order on as the env layer sets them."""
    def conf(p):
        p.set_stream_slices(slices); p.set_split_position_stage(True); p.set_fused_substeps(False)
        p.set_lazy_position_stage(True); p.set_cost_ordered_launch(True)
    run_pair(hull_scene(), E, configure=conf, bounds=slice_bounds(E, slices) if E >= 1024 else None)


# ---------------------------------------------------------------------------------------------------- fallbacks
@pytest.mark.gpu
def test_tree_offsets_turn_the_snapshot_off():
    """Per-env root offsets make reset states differ: after rp_set(RP_TREE_OFFSET) a reset env goes through the leading
    stage again (a snapshot copy would publish the site positions of the unshifted hands)."""
    si = hull_scene()
    E = 8
    off = np.zeros((E, 2, 3))
    off[:, :, 1] = 0.004 * (np.arange(E)[:, None] - 3)
    off[:, 0, 2] = -0.002 * np.arange(E)

    def between(p, t, i):
        if t == 2:
            p.set(engine.TREE_OFFSET, off)
    a, b = run_pair(si, E, configure=lazy, between=between)
    sx = a.get(engine.SITE_XPOS)
    assert not np.array_equal(sx[0], sx[7])


@pytest.mark.gpu
def test_qpos_written_between_reset_and_step():
    """rp_reset, then RP_QPOS written, then rp_step: the write clears the validity the snapshot gave, the ordinary
    stage runs for the new state."""
    si = hull_scene()
    E = 8
    rows = replay_ctrl(si)
    a, b = make_pair(si, E, configure=lazy)
    for t in range(6):
        c = ctrl_at(rows, t, E)
        for p in (a, b):
            p.set(engine.CTRL, c)
            if t in (2, 4):
                mask = np.zeros(E, np.uint8); mask[[1, 6]] = 1
                p.reset(mask)
            if t == 2:
                q = p.qpos
                q[6, :20] += 0.01 * np.random.default_rng(7).standard_normal(20)
                p.set(engine.QPOS, q)
            p.step(NSUB)
        assert_equal_state(a, b, ("step", t))


@pytest.mark.gpu
def test_option_setter_between_two_resets_rebuilds_the_snapshot():
    """rp_set_mpr_tolerance between two resets: the second reset copies a snapshot built with the new tolerance, equal to
    what the recomputed stage gives."""
    def between(p, t, i):
        if t == 3:
            p.set_mpr_tolerance(1e-6, 1e-10)
        if t == 5:
            p.set_lean_solver(40)
    run_pair(hull_scene(), 8, configure=split_stage, between=between)


@pytest.mark.gpu
def test_legacy_step_false_keeps_its_leading_stage():
    def conf(p):
        one_kernel(p); p.set_legacy_step(False); p.set_lazy_position_stage(True)
    run_pair(hull_scene(), 8, configure=conf)


@pytest.mark.gpu
def test_reset_then_forward_then_step():
    """env.reset()'s sequence, rp_reset + rp_forward, and a masked rp_reset followed by a plain rp_step."""
    si = hull_scene()
    E = 8
    rows = replay_ctrl(si)
    a, b = make_pair(si, E, configure=lazy_split_ordered)
    for t in range(8):
        c = ctrl_at(rows, t, E)
        for p in (a, b):
            p.set(engine.CTRL, c)
            if t == 3:
                p.reset(None); p.forward()
            if t == 5:
                mask = np.zeros(E, np.uint8); mask[[0, 7]] = 1
                p.reset(mask)
            p.step(NSUB)
        assert_equal_state(a, b, ("step", t))


# ---------------------------------------------------------------------------------------------------- captured graph
@pytest.mark.gpu
def test_captured_step_with_a_reset_mask_replays_like_the_eager_run():
    """A step with a reset mask captured after the snapshot exists and replayed twice, against the eager run with the
    switch off; then tree offsets are set and the SAME graph is replayed: its reset falls back to the leading stage."""
    import torch
    si = hull_scene()
    E = 8
    rows = replay_ctrl(si)
    a, b = make_pair(si, E, configure=lazy)
    eager = torch.cuda.current_stream().cuda_stream
    a.set_stream(eager)   # (as suite.physics.TorchPhysics: the engine enqueues on torch's stream, which the capture replaces)
    masks = _Masks()
    for t in range(3):
        for p in (a, b):
            p.set(engine.CTRL, ctrl_at(rows, t, E)); p.step(NSUB)
    mask = np.zeros(E, np.uint8); mask[[2, 5]] = 1
    step_masked(a, masks, mask); step_masked(b, masks, mask)   # (the snapshot exists from here on)
    assert_equal_state(a, b, "eager masked step")
    dm = masks.device(mask)
    a.sync()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    try:
        with torch.cuda.graph(g):
            a.set_stream(torch.cuda.current_stream().cuda_stream)
            a.step_masked(NSUB, None, dm)
    finally:
        a.set_stream(eager)
    for r in range(2):
        g.replay(); torch.cuda.synchronize()
        step_masked(b, masks, mask)
        assert_equal_state(a, b, ("replay", r))
    off = np.zeros((E, 2, 3)); off[:, :, 1] = 0.003 * np.arange(E)[:, None]
    for p in (a, b):
        p.set(engine.TREE_OFFSET, off)
    a.sync()
    g.replay(); torch.cuda.synchronize()
    step_masked(b, masks, mask)
    assert_equal_state(a, b, "replay after tree offsets")
