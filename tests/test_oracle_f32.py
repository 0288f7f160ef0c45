"""The float32 build of the oracle (oracle/librp_oracle_f32.so, Oracle(precision=32)) as a yardstick: host checks, no GPU.

It is a restatement of the fp64 oracle in float32 -- the fp32 engine's bars are multiples of ITS error
(tests/test_gpu_parity_fp32.py) -- so it must itself behave like the fp64 oracle on every window those tests use: teacher
forced from the fp64 oracle's states it raises no warning, needs at most 2 Newton iterations more or fewer, and sees the
same number of contacts on all but at most 2 steps of a window.  These are conditions on the reference alone: a window
that fails them is replaced, the conditions stay."""
import warnings

import numpy as np
import pytest

import test_gpu_parity as P
import test_gpu_parity_fp32 as F


def _two_hands():
    return F._scene(primitive_fingertip_collisions=True)


def test_float32_oracle_has_float32_views_and_the_fp64_one_is_untouched():
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    si = _two_hands()
    blob = engine.make_blob(si.model, si.key_joint_ids)
    o64, o32 = Oracle(si.model, blob), Oracle(si.model, blob, precision=32)
    for name in ("qpos", "qvel", "ctrl", "xpos", "qM", "body_pos", "sensor_torque"):
        assert o64.view(name).dtype == np.float64 and o32.view(name).dtype == np.float32, name
        assert o64.view(name).shape == o32.view(name).shape
    # the blob's float64 tables are converted at load: the reset state is the fp64 one rounded once
    assert np.array_equal(o32.qpos, o64.qpos.astype(np.float32))
    assert np.array_equal(o32.body_pos, o64.body_pos.astype(np.float32))
    np.testing.assert_allclose(o32.xpos, o64.xpos, rtol=0, atol=2e-6)
    assert o32.ncon == o64.ncon and o32.nefc == o64.nefc and o32.warnings == 0
    with pytest.raises(ValueError):
        Oracle(si.model, blob, precision=16)


def test_float32_oracle_follows_the_fp64_one_on_the_existing_fp32_stream():
    """The stream of test_teacher_forced_fp32_random_targets: median 3.5e-6, worst 1.3e-3 of the step's velocity change --
    far below the fp32 contract's 5e-3, so 8 x the restatement is a tighter bar than the contract on the median."""
    si = _two_hands()
    rec = P.Fp32Record(si)
    P.teacher_forced(si, None, P.ctrl_sequence(si.model, 300, 1), record=rec)
    r = np.asarray(rec.ref_all)
    print("float32 oracle, random targets: worst %.2e median %.2e p90 %.2e" % (r.max(), np.median(r), np.percentile(r, 90)))
    assert rec.steps == 300 and rec.warnings == 0 and rec.ncon_diff == 0
    assert r.max() < P.FP32_WORST and P.FP32_MARGIN * np.median(r) < P.FP32_WORST / 10


@pytest.mark.parametrize("name", list(F.SCENES))
def test_float32_oracle_is_sound_on_the_window(name):
    rec, info = F.SCENES[name](None, P.Fp32Record)
    r = np.asarray(rec.ref_all)
    print(name, info, "steps", rec.steps, "Newton iterations differ by <=", rec.iter_diff, "contact counts differ on", rec.ncon_diff,
          "worst/median/p90 %.2e %.2e %.2e" % (r.max(), np.median(r), np.percentile(r, 90)))
    assert rec.steps >= 10
    rec.assert_restatement_is_sound(name)
    assert r.max() < P.FP32_WORST, "a window on which float32 itself misses the fp32 contract cannot gate the engine"


def test_float32_oracle_is_sound_on_the_sensor_window():
    o = F.sensors(_two_hands(), None)
    o["rec"].assert_restatement_is_sound("sensors")
    assert o["scale"] > 0.05 and o["touched"] >= 3
    assert max(o["ref_t"]) < P.FP32_WORST * max(1.0, o["scale"]) and np.isfinite(o["ref_f"]).all()


def test_the_capacity_sweep_has_enough_poses_on_either_side():
    """What the oracle alone guarantees about test_fp32_capacity_flag_rules_over_hand_in_hand_poses: at least 8 poses within
    both fp32 capacities with more than 8 contacts (no flag allowed there) and at least 8 with more than 32 contacts (a flag
    is certain there)."""
    rec, st = F.capacity_sweep(_two_hands(), None)
    print({k: v for k, v in st.items() if not isinstance(k, tuple)})
    assert st["within_over_8"] >= 8 and st["beyond_contacts"] >= 8, st
    rec.assert_restatement_is_sound("capacity sweep")


def test_float32_oracle_sees_the_overflow_poses_like_the_fp64_one():
    """The poses of test_fp32_contact_capacity_overflow_keeps_the_deepest_contacts: same contact count, and distances whose
    float32 error sets that test's tolerance."""
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    si = _two_hands()
    blob = engine.make_blob(si.model, si.key_joint_ids)
    o64, o32 = Oracle(si.model, blob), Oracle(si.model, blob, precision=32)
    for dx in F.OVERFLOW_DX:
        F.hands_pushed_together(si, o64, dx); F.hands_pushed_together(si, o32, dx)
        assert o64.ncon > 32 and o32.ncon == o64.ncon, (o64.ncon, o32.ncon)
        d64 = np.sort(o64.contact.reshape(-1, 16)[:, 0])
        d32 = np.sort(o32.contact.reshape(-1, 16)[:, 0].astype(np.float64))
        tol = F.overflow_tolerance(d64, d32, 32)
        print("dx", dx, "contacts", o64.ncon, "tolerance %.2e" % tol, "gap below the 32nd deepest %.2e" % (d64[32] - d64[31]))
        assert tol < 1e-6, tol   # (float32-sized: a few roundings of centimetre depths)
