"""The fp32 engine (Engine<float>: its own one-kernel position stage, solver launch bounds, WIDE dense step and
capacities of 32 contacts / 240 Jacobian entries / 56 dense rows) against the oracle, teacher forced, on every kind of
scene the fp64 build is gated on.

Per step the fp32 engine and the float32 RESTATEMENT of the oracle (Oracle(precision=32): the same formulae with every
stored value, constant, product and library call in float32 -- oracle/rp_oracle.c) both start from the fp64 oracle's
state, and both results are compared with the fp64 oracle's, relative to the step's largest velocity change.  Bars:
  * worst step < 5e-3: the fp32 contract of tests/test_gpu_parity.py, unchanged;
  * median and 90th percentile <= 8 x the restatement's on the same steps (the project's margin over a float32
    restatement: tests/test_gpu_learn.py, test_gpu_offpolicy.py, test_gpu_droq.py);
  * the contacts' geom pairs equal and no warn flag; a step is left out only if the contact counts differ and at least
    as many contacts lie within 1e-6 (the fp32 engine's MPR floor) of the dist = 0 threshold, at most 2 per scene.
No engine-measured number is a bar.  The conditions on the restatement itself (no warnings, Newton iterations within 2,
contact counts equal on all but 2 steps) are checked without a GPU, on the same windows, by tests/test_oracle_f32.py.

The capacity rules of the fp32 build (rp_dim "max_contacts" / "max_entries"; test_fp32_capacity_*):
  * a step whose two position stages see no more than max_contacts contacts in the oracle and whose entry upper bound is
    within max_entries raises no flag;
  * a step without a flag meets the bars above: capacity is never lost silently;
  * beyond the capacity RP_WARN_CONTACT_FULL is raised, the deepest contacts are kept (NCON = max_contacts), the state stays
    finite; slots of CONTACT_DIST / CONTACT_GEOMS from NCON to 63 hold 0 and (-1, -1).

SCENES maps a name to a function (precision, record) -> info: precision 32 runs the engine, None the oracles alone.
"""
import warnings

import numpy as np
import pytest

import test_gpu_parity as P

pytestmark = pytest.mark.gpu


def _scene(**kw):
    from robopianist_amd.model import scene
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return scene.build_scene(gravity_compensation=True, **kw)


SIX = ("forearm_tx", "forearm_ty", "forearm_tz", "forearm_roll", "forearm_pitch", "forearm_yaw")
TOPOLOGIES = {   # the scenes of test_teacher_forced_fp64_other_topologies (generic solver build, fused segments, deep builds)
    "right hand only": dict(hands=("right",)),
    "no forearm dofs": dict(forearm_dofs=()),
    "reduced action space": dict(reduced_action_space=True),
    "rotational forearm dofs": dict(forearm_dofs=("forearm_roll", "forearm_pitch")),
    "reduced, left hand, tz + yaw": dict(hands=("left",), reduced_action_space=True, forearm_dofs=("forearm_tz", "forearm_yaw")),
    "three forearm dofs, reduced": dict(reduced_action_space=True, forearm_dofs=("forearm_tx", "forearm_ty", "forearm_yaw")),
    "two hands, four forearm dofs": dict(forearm_dofs=("forearm_tx", "forearm_ty", "forearm_roll", "forearm_yaw")),
    "right hand, all six forearm dofs": dict(hands=("right",), forearm_dofs=SIX),
    "left hand, five forearm dofs": dict(hands=("left",), forearm_dofs=SIX[1:]),
}


def _replay_window(lo, hi, min_contacts, **kw):
    def run(precision, record_of):
        si = _scene(**kw)
        rec = record_of(si)
        _, maxcon = P.teacher_forced(si, precision, P._replay_ctrl(si)[lo:hi], record=rec)
        assert maxcon >= min_contacts, maxcon
        return rec, {"max contacts": maxcon}
    return run


def _topology(kw, seed=3, nsteps=120):
    def run(precision, record_of):
        si = _scene(primitive_fingertip_collisions=True, **kw)
        rec = record_of(si)
        _, maxcon = P.teacher_forced(si, precision, P.ctrl_sequence(si.model, nsteps, seed), record=rec)
        return rec, {"max contacts": maxcon, "nv": int(si.model.nv)}
    return run


def _both_hands_six_dofs(precision, record_of):
    """2 x (24 + 6) hand dofs (nv 148: four solver slots for touched keys are left): random finger targets with the
    forearms lifted off the keys and rolled / yawed a little (test_both_hands_with_all_six_forearm_dofs_build_and_step)."""
    si = _scene(primitive_fingertip_collisions=True, forearm_dofs=SIX)
    m = si.model
    ctrl = P.ctrl_sequence(m, 100, 3)
    for a, n in enumerate(m.names["actuator"]):
        if n.endswith("forearm_ty"):
            ctrl[:, a] = m.actuator_ctrlrange[a, 1]
        elif n.split("/")[-1].startswith("forearm_"):
            ctrl[:, a] = np.clip(0.1 if n.endswith(("forearm_roll", "forearm_yaw")) else 0.0, *m.actuator_ctrlrange[a])
    rec = record_of(si)
    _, maxcon = P.teacher_forced(si, precision, ctrl, record=rec)
    return rec, {"max contacts": maxcon, "nv": int(m.nv)}


def _cylinders(precision, record_of):
    """Wrist / knuckle colliders as cylinders next to hull fingertips (MESH = 2 builds, every cylinder pair through the portal
    refinement), the hands pushed into each other just far enough to stay within the fp32 capacity on about half of the
    poses.  stable_only: a pose is compared only if the fp64 oracle's own contact depths move by less than 1e-6 under a
    1e-7 perturbation of qpos -- the size of rounding qpos to float32 (P.pile_up explains the cylinder's branches)."""
    si = _scene(primitive_fingertip_collisions=False, cylinder_colliders=True, impratio=10.0)
    rec, st = record_of(si), {}
    P.pile_up(si, 100, seed=4, lo_dx=0.072, hi_dx=0.082, stable_only=True, stats=st, precision=precision, record=rec)
    cyl = sum(v for k, v in st.items() if isinstance(k, tuple) and 5 in k)
    assert st.get("compared", 0) >= 20 and cyl >= 12, st
    return rec, {"compared": st.get("compared", 0), "cylinder contacts": cyl, "flagged": st.get("flagged", 0),
                 "unstable": st.get("unstable", 0)}


def _palm_flat(precision, record_of):
    si = _scene(primitive_fingertip_collisions=True)
    rec = record_of(si)
    # (a little shallower than the fp64 test's poses: those mostly exceed 32 contacts)
    _, maxcon, pairs, most = P.palm_flat(si, 40, precision=precision, record=rec, dz_range=(0.094, 0.097))
    assert pairs >= 20 and most >= 4, (pairs, most)
    return rec, {"max contacts": maxcon, "box-box pairs with > 3 points": pairs, "most points": most}


def _box_box(precision, record_of):
    si = _scene(primitive_fingertip_collisions=True)
    rec = record_of(si)
    _, boxbox, maxcon, flags = P.box_box_drive(si, precision, record=rec, nsteps=240)
    assert boxbox >= 50 and flags == 0, (boxbox, flags)
    return rec, {"max contacts": maxcon, "box-box contacts": boxbox}


def _dense_block(precision, record_of):
    """Hand-in-hand poses within the fp32 capacity: most contacts couple the two chains, so the solver's dense cross-chain
    block -- and with it dense_factor_solve<float>'s four-column WIDE step and its pair / single remainders -- has real
    size.  At least 12 contacts must be reached."""
    si = _scene(primitive_fingertip_collisions=True)
    rec, st = record_of(si), {}
    _, maxcon, maxent, _ = P.pile_up(si, 60, seed=7, lo_dx=0.066, hi_dx=0.080, stats=st, precision=precision, record=rec)
    assert maxcon >= 12, maxcon
    return rec, {"max contacts": maxcon, "max entries": maxent, "flagged": st.get("flagged", 0)}


SCENES = {
    "hull fingertips, replay 420-620": _replay_window(420, 620, 6, primitive_fingertip_collisions=False),
    "200-vertex hulls, replay 400-480": _replay_window(400, 480, 4, primitive_fingertip_collisions=False, mesh_colliders=200),
    "cylinder colliders, hand in hand": _cylinders,
    "box-box, palm flat on the keys": _palm_flat,
    "box-box, hands driven together": _box_box,
    "impratio 1, replay 520-700": _replay_window(520, 700, 6, primitive_fingertip_collisions=True, impratio=1.0),
    "impratio 10, replay 520-700": _replay_window(520, 700, 6, primitive_fingertip_collisions=True, impratio=10.0),
    "dense cross-chain block": _dense_block,
    "both hands, all six forearm dofs": _both_hands_six_dofs,
}
# (random targets of seed 3, 120 steps; on the six-dof right hand that stream has a step where the restatement needs three
# Newton iterations more than the fp64 oracle, which tests/test_oracle_f32.py does not admit in a window: seed 9 there)
# (... and with four forearm dofs on two hands seed 3 drives the hands into each other: 19 contacts of ~16 entries each,
# beyond the fp32 build's 240 entries -- RP_WARN_CONTACT_FULL, rightly: seed 8 there, 13 contacts)
TOPOLOGY_STREAMS = {"right hand, all six forearm dofs": (9, 100), "two hands, four forearm dofs": (8, 120)}
SCENES.update({"topology: " + k: _topology(v, *TOPOLOGY_STREAMS.get(k, ())) for k, v in TOPOLOGIES.items()})


@pytest.mark.parametrize("name", list(SCENES))
def test_fp32_teacher_forced_against_the_restatement(name):
    rec, info = SCENES[name](32, P.Fp32Record)
    print("fp32", name, info)
    rec.assert_bars(name)


def sensors(si, precision, nsteps=160):
    """Joint torque and touch sensors (test_torque_and_touch_sensors_match_the_oracle), the engine and the restatement
    from the same states.  Returns per-step worst |d torque| and |d touch| of both, the torque scale and the touches."""
    from robopianist_amd import engine
    from robopianist_amd.model import engine_tables
    m = si.model
    phys, orc = P.make_pair(si, precision, nenv=1)
    rec = P.Fp32Record(si)
    if phys is not None:
        phys.set_acc_sensors(True)
    site_ids = engine_tables.build_engine_tables(m, si.key_joint_ids)["eng_site_modelid"]
    keys = set(int(k) for k in si.key_joint_ids)
    hand = np.array([j for j in range(m.nv) if j not in keys])
    out = {"eng_t": [], "ref_t": [], "eng_f": [], "ref_f": [], "scale": 0.0, "touched": 0, "rec": rec}
    # (seed 8: on the fp64 test's stream, seed 7, the restatement needs three Newton iterations more on one step, which
    # tests/test_oracle_f32.py does not admit in a window)
    for c in P.ctrl_sequence(m, nsteps, 8):
        if phys is not None:
            phys.set(engine.QPOS, orc.qpos[None, :]); phys.set(engine.QVEL, orc.qvel[None, :])
            phys.set(engine.QACC_WARMSTART, orc.qacc_warmstart[None, :]); phys.set(engine.CTRL, c[None, :])
        rec.restate(orc, orc.qpos, orc.qvel, orc.qacc_warmstart, c)
        orc.ctrl[:] = c
        v0 = orc.qvel.copy()
        if phys is not None:
            phys.step(1)
        orc.step(1)
        rec.compare(orc, v0)
        want_t, want_f = orc.sensor_torque[hand], orc.sensor_touch[site_ids]
        out["ref_t"].append(np.abs(rec.o32.sensor_torque[hand].astype(np.float64) - want_t).max())
        touching = bool((want_f > 0).any())   # (most steps touch nothing: the touch figures are over the steps that do)
        if touching:
            out["ref_f"].append(np.abs(rec.o32.sensor_touch[site_ids].astype(np.float64) - want_f).max())
        out["scale"] = max(out["scale"], float(np.abs(want_t).max()))
        out["touched"] += int((want_f > 0).sum())
        if phys is not None:
            assert phys.warn_flags.max() == 0
            tq = phys.get(engine.SENSOR_TORQUE).astype(np.float64)[0]
            out["eng_t"].append(np.abs(tq[hand] - want_t).max())
            d_f = np.abs(phys.get(engine.SENSOR_TOUCH).astype(np.float64)[0] - want_f).max()
            if touching:
                out["eng_f"].append(d_f)
            assert np.abs(tq[np.asarray(si.key_joint_ids)]).max() == 0.0
    return out


def test_fp32_torque_and_touch_sensors_against_the_restatement():
    """The fp32 sensor stage.  Bars, derived like the state's: worst |d torque| < 5e-3 of the largest torque of the run,
    worst |d touch| < 5e-3 of the largest touch force; median and p90 of both <= 8 x the restatement's sensor errors."""
    si = _scene(primitive_fingertip_collisions=True)
    o = sensors(si, 32)
    assert o["scale"] > 0.05 and o["touched"] >= 3 and len(o["eng_f"]) >= 10, (o["scale"], o["touched"], len(o["eng_f"]))
    for kind, scale in (("t", max(1.0, o["scale"])), ("f", 1.0)):
        e, r = np.asarray(o["eng_" + kind]), np.asarray(o["ref_" + kind])
        print("fp32 sensors %s: engine worst/median/p90 %.2e %.2e %.2e | restatement %.2e %.2e %.2e"
              % ("torque" if kind == "t" else "touch", e.max(), np.median(e), np.percentile(e, 90), r.max(), np.median(r), np.percentile(r, 90)))
        assert e.max() < P.FP32_WORST * scale, (kind, e.max())
        assert np.median(e) <= P.FP32_MARGIN * np.median(r), (kind, np.median(e), np.median(r))
        assert np.percentile(e, 90) <= P.FP32_MARGIN * np.percentile(r, 90), (kind,)


# ---- the fp32 capacities ------------------------------------------------------------------------------------------
CAPACITY_POSES = dict(nsteps=60, seed=9, lo_dx=0.06, hi_dx=0.10)


def capacity_sweep(si, precision, nsteps=CAPACITY_POSES["nsteps"]):
    """~60 hand-in-hand poses from a few to far more than 32 contacts (P.pile_up states the rules it asserts per pose).
    Returns (record, stats)."""
    rec, st = P.Fp32Record(si), {}
    kw = dict(CAPACITY_POSES, nsteps=nsteps)
    P.pile_up(si, stats=st, precision=precision, record=rec, **kw)
    return rec, st


def test_fp32_capacity_flag_rules_over_hand_in_hand_poses():
    si = _scene(primitive_fingertip_collisions=True)
    rec, st = capacity_sweep(si, 32)
    print("fp32 capacity sweep:", {k: v for k, v in st.items() if not isinstance(k, tuple)})
    assert st.get("unflagged_over_8", 0) >= 8 and st.get("flagged", 0) >= 8, st
    rec.assert_bars("capacity sweep, unflagged poses")


OVERFLOW_DX = (0.10, 0.12, 0.14)


def hands_pushed_together(si, orc, dx):
    """The pose of the fp64 overflow test (forearms shifted by dx towards each other) with the hand joints moved off their
    reset values by a seeded 0.05 rad: in the reset posture the fingers' capsules are exactly parallel, and whether a
    parallel pair gives one contact or two is decided by the rounding of 1 - cos^2 in float32 -- in the restatement as in
    any fp32 implementation (it sees 88 contacts where the fp64 oracle sees 69)."""
    m = si.model
    rng = np.random.default_rng(int(round(dx * 1000)))
    orc.reset()
    q = orc.qpos.astype(np.float64)
    for i, n in enumerate(m.names["joint"]):
        if n.split("/")[-1] == "forearm_tx":
            q[i] += -dx if n.startswith("rh") else dx
        elif "shadow_hand" in n and n.split("/")[-1] != "forearm_ty":
            q[i] = np.clip(q[i] + rng.normal(0, 0.05), *m.jnt_range[i])
    orc.qpos[:] = q
    orc.forward()
    return q


def overflow_tolerance(d64, d32, cap):
    """How far the float32 restatement's contact distances are from the fp64 oracle's `cap` deepest ones (for each of
    those, the nearest of the restatement's), times the standing margin 8; never below one float32 rounding of the
    deepest distance."""
    near = max(np.abs(d32 - d).min() for d in d64[:cap])
    return max(P.FP32_MARGIN * near, float(np.spacing(np.float32(np.abs(d64).max()))))


def test_fp32_contact_capacity_overflow_keeps_the_deepest_contacts():
    """The twin of test_contact_capacity_overflow_keeps_the_deepest_contacts at the fp32 capacity: NCON = max_contacts (32),
    RP_WARN_CONTACT_FULL, the kept distances are the oracle's deepest ones -- to the float32 restatement's own error on
    these distances (8 x its largest, and never less than one float32 rounding of the deepest) -- the readback slots from
    NCON to 63 hold dist 0 and geoms (-1, -1), and the state stays finite over 10 more steps."""
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    si = _scene(primitive_fingertip_collisions=True)
    phys, orc = P.make_pair(si, 32, nenv=1)
    o32 = Oracle(si.model, phys.blob, precision=32)
    cap = phys.dim("max_contacts")
    assert cap == phys.max_contacts == 32 and phys.dim("max_entries") == 240 and phys.dim("max_dense_rows") == 56
    assert engine.MAX_CONTACTS == 64
    for dx in OVERFLOW_DX:
        q = hands_pushed_together(si, orc, dx)
        hands_pushed_together(si, o32, dx)
        assert orc.ncon > cap and o32.ncon == orc.ncon, (orc.ncon, o32.ncon)
        d64 = np.sort(orc.contact.reshape(-1, 16)[:, 0])
        d32 = np.sort(o32.contact.reshape(-1, 16)[:, 0].astype(np.float64))
        tol = overflow_tolerance(d64, d32, cap)
        phys.reset()
        phys.set(engine.QPOS, q[None, :])
        phys.forward()
        ncon = int(phys.get(engine.NCON)[0])
        assert ncon == cap
        assert int(phys.warn_flags.max()) & engine.WARN_CONTACT_FULL
        dist = phys.get(engine.CONTACT_DIST)[0].astype(np.float64)
        geoms = phys.get(engine.CONTACT_GEOMS)[0]
        print(f"fp32 overflow dx {dx}: oracle contacts {orc.ncon}, kept {ncon}, tolerance {tol:.2e}, "
              f"worst |d dist| {np.abs(np.sort(dist[:ncon]) - d64[:cap]).max():.2e}")
        np.testing.assert_allclose(np.sort(dist[:ncon]), d64[:cap], rtol=0, atol=tol)
        assert (dist[ncon:] == 0).all() and (geoms[ncon:] == -1).all() and (geoms[:ncon] >= 0).all()
        phys.step(10)
        assert np.isfinite(phys.qpos).all() and np.isfinite(phys.qvel).all()


def short_window(si, kind, n):
    """A short window of one scenario with its bars asserted, for the emulator twins (tests/test_wavesim.py), which pass the
    scene.  Returns (steps compared, largest contact count, engine worst / median / p90, restatement worst / median / p90,
    flagged poses, unflagged poses with more than 8 contacts)."""
    rec, st = P.Fp32Record(si), {}
    if kind == "replay":
        P.teacher_forced(si, 32, P._replay_ctrl(si)[420:420 + n], record=rec)
    elif kind == "cylinder":
        P.pile_up(si, n, seed=4, lo_dx=0.072, hi_dx=0.082, stable_only=True, stats=st, precision=32, record=rec)
    elif kind == "palm":
        P.palm_flat(si, n, precision=32, record=rec, dz_range=(0.094, 0.097))
    elif kind == "capacity":
        P.pile_up(si, stats=st, precision=32, record=rec, **dict(CAPACITY_POSES, nsteps=n))
    else:
        raise ValueError(kind)
    f = rec.assert_bars(kind)
    return (f["steps"], rec.maxcon) + f["engine"] + f["restatement"] + (st.get("flagged", 0), st.get("unflagged_over_8", 0))
