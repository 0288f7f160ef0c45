"""The solver and narrow-phase settings that no other test moves off their defaults: the model options opt_tolerance /
opt_iterations / opt_ls_iterations / opt_ls_tolerance (read from the blob) and the run-time setters rp_set_solver_limits,
rp_set_solver_tolerance and rp_set_mpr_tolerance.  Four code paths run here and nowhere else: a Newton solve that ends on
its iteration cap, a line search that ends on its evaluation cap, a solve under a looser tolerance, and the
`tol_poly != tol` branch of the portal refinement (csrc/rp_narrow.hpp).

Every scenario is TEACHER-FORCED from a default-settings oracle's trajectory along the headline replay: each compared
step starts from that oracle's (qpos, qvel, qacc_warmstart), so the states stay sane whatever the option does to the one
step under comparison (a solver capped at 3 iterations left to run free leaves the piano within 70 steps).  A second
oracle takes such a state through qpos / qvel / qacc_warmstart and step1(): rpo_step runs mj_step2 on the stage data in
place, and step1() recomputes them without touching qacc_warmstart (forward() would overwrite it with its own solve).

  A   a setter equals the model option, bit for bit: an engine built from a copy of the model with the opt_* values
      changed against a default-model engine given the setter call -- qpos, qvel, NCON, CONTACT_DIST, QACC_WARMSTART.
      Conditions: the engine under test differs from a default engine on at least one step (the knob did something); where
      the Newton cap is set, the default oracle needed more iterations than the cap on at least 10 of the compared steps
      (the cap bound).  A line-search cap alone leaves the Newton cap at 100, which no step reaches: there the first
      condition is the only one.
  B   the same settings against the oracle built from the same modified model, at the fp64 bar of tests/test_gpu_parity.py:
      relative dv < 1e-9, equal contact counts by teacher_forced's on-threshold rule.
  C1  rp_set_mpr_tolerance's contract table (include/rp_engine.h), every row by bit-identity against an engine given the
      explicit equivalent pair.  The polytope tolerance decides hull-box / hull-hull pairs (hull fingertips); `tolerance`
      itself decides only the other MPR pairs, so those rows run with the wrist / knuckle colliders as cylinders.
  C2  fp32 engines clamp both tolerances at 1e-6.
  C3  the refined rule (polytope pairs at 1e-10) against the oracle's refined rule at the mj_steps of the hull replay
      where the oracle's two rules differ by more than 1e-9 of the step's velocity change (found with the oracle alone:
      REFINED_STEPS) -- elsewhere polytope pairs stop on a face either way and a parity run cannot tell whether the
      branch ran.  Condition: the uniform engine differs from the refined engine at every such step.

Figures of the GPU run (MI355X; the whole output is profiles/solver_options_gpu_tests.txt), worst relative dv:
  B   limits (4, 6): capsule 5.11e-12, hull 1.09e-11; tolerance (1e-3, 0.3): capsule 3.92e-12, hull 5.45e-12
      (wave emulator: 8.87e-12, 5.71e-12, 4.04e-12, 2.80e-12)
  C3  refined engine against refined oracle: hull 4.56e-13, 200-vertex hulls 9.54e-14; the uniform engine is 5.1e-2 / 8.0e-3
      of the velocity change away at the closest of those steps
  A, C1, C2: every bit-identity holds; each setting moves 27 to 69 of the 70 steps, the line-search tolerance alone 3 or 4
  (see _WINDOW)

No torch in here: the file also runs against the wave-emulator build (RP_ENGINE_LIB, tests/wavesim; the CPU twin is
tests/test_wavesim.py::test_solver_and_mpr_options_on_the_wave_emulator)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SCENES = {
    "capsule": dict(primitive_fingertip_collisions=True),
    "hull": dict(primitive_fingertip_collisions=False),
    "cylinder": dict(primitive_fingertip_collisions=False, cylinder_colliders=True),   # hull tips, cylinder knuckles
    "mesh200": dict(primitive_fingertip_collisions=False, mesh_colliders=200),         # the graph walk of model/hull.py
}
_scene_cache, _traj_cache = {}, {}

# Window of the replay (rows of the per-mj_step control array) every windowed scenario compares by default.
LO, N = 400, 70

# mj_steps of the 1580-step replay (0-based rows of the per-mj_step control array) at which the ORACLE's step under the
# refined rule differs from its step under the uniform rule by more than 1e-9 of the step's velocity change.  Searched
# with the oracle alone over the whole replay: hull fingertips 2 steps of 1580 (5.1e-2 and 6.8e-2 of the velocity change);
# 200-vertex hulls 28 steps, the first three of which are used.
REFINED_STEPS = {"hull": (1170, 1287), "mesh200": (204, 312, 319)}


def _scene(name):
    if name not in _scene_cache:
        from robopianist_amd.model import scene
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _scene_cache[name] = scene.build_scene(gravity_compensation=True, **_SCENES[name])
    return _scene_cache[name]


def _replay_ctrl(si):
    """The headline replay's controls, one row per mj_step (tests/test_gpu_parity.py: _replay_ctrl)."""
    m = si.model
    a = np.load("tests/golden/twinkle_twinkle_actions.npy").astype(np.float64)[:, :-1]
    lo, hi = m.actuator_ctrlrange[:, 0], m.actuator_ctrlrange[:, 1]
    return np.repeat(lo + (np.clip(a, -1, 1) + 1.0) * 0.5 * (hi - lo), 10, axis=0)


def _trajectory(si, upto):
    """The default-settings oracle run free along the replay, computed once per scene and only ever extended: row i holds
    the state BEFORE mj_step i as (qpos, qvel, qacc_warmstart, ctrl), iters[i] the Newton iterations of mj_step i.
    Returns (rows, iters, the oracle's warnings)."""
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    t = _traj_cache.get(id(si))
    if t is None:
        t = _traj_cache[id(si)] = dict(si=si, orc=Oracle(si.model, engine.make_blob(si.model, si.key_joint_ids)),
                                       ctrl=_replay_ctrl(si), rows=[], iters=[])
    orc = t["orc"]
    while len(t["rows"]) < upto:
        c = t["ctrl"][len(t["rows"])]
        t["rows"].append((orc.qpos.copy(), orc.qvel.copy(), orc.qacc_warmstart.copy(), c.copy()))
        orc.ctrl[:] = c
        orc.step(1)
        t["iters"].append(orc.solver_iter)
    return t["rows"], np.asarray(t["iters"]), orc.warnings


def _engine(si, precision, E, model=None):
    """An engine of the scene's model, or of `model` (a copy with other options: no fp32-against-fp64 build self-check of
    its own, the default-model engines of the same scenario have run it)."""
    from robopianist_amd import engine
    return engine.BatchedPhysics(si.model if model is None else model, si.key_joint_ids, n_envs=E, precision=precision,
                                 self_check=None if model is None else False)


def _put(phys, row):
    from robopianist_amd import engine
    q, v, w, c = row
    phys.set(engine.QPOS, q[None, :]); phys.set(engine.QVEL, v[None, :])
    phys.set(engine.QACC_WARMSTART, w[None, :]); phys.set(engine.CTRL, c[None, :])


def _put_oracle(orc, row):
    q, v, w, c = row
    orc.qpos[:] = q; orc.qvel[:] = v; orc.qacc_warmstart[:] = w; orc.ctrl[:] = c
    orc.step1()


def _bits(phys):
    """The compared outputs as bytes: equal bits, and a NaN compares equal to the same NaN."""
    from robopianist_amd import engine
    return tuple(phys.get(f).tobytes() for f in (engine.QPOS, engine.QVEL, engine.NCON, engine.CONTACT_DIST, engine.QACC_WARMSTART))


_OPTION = {"limits": ("opt_iterations", "opt_ls_iterations", int, "set_solver_limits"),
           "tolerance": ("opt_tolerance", "opt_ls_tolerance", float, "set_solver_tolerance")}


def _model_with(si, kind, calls):
    """A copy of the scene's model whose opt_* values are what the setter calls leave behind (values <= 0 keep the
    current setting)."""
    from robopianist_amd.model import compile as mcompile
    m = mcompile.Model(si.model)
    k0, k1, typ, _ = _OPTION[kind]
    for a, b in calls:
        if a > 0: m[k0] = typ(a)
        if b > 0: m[k1] = typ(b)
    return m


def _apply(phys, kind, calls):
    for a, b in calls:
        getattr(phys, _OPTION[kind][3])(a, b)


def setter_equals_model_option(si, precision, kind, calls, lo=LO, n=N, E=2):
    """Part A.  `calls`: the (a, b) argument pairs given to the setter, in order.  Returns (steps at which the setter engine
    and the model-built engine differ in any bit, steps at which the setter engine differs from a default engine, steps at
    which the default oracle needed more Newton iterations than the cap the calls leave -- 0 if they leave the Newton cap
    alone --, non-finite values in the setter engine's state, the largest warn flag, the oracle's warnings)."""
    rows, iters, owarn = _trajectory(si, lo + n)
    model = _model_with(si, kind, calls)
    built, under_test, default = _engine(si, precision, E, model), _engine(si, precision, E), _engine(si, precision, E)
    _apply(under_test, kind, calls)
    mismatch = differs = nonfinite = warn = 0
    for row in rows[lo:lo + n]:
        out = []
        for p in (built, under_test, default):
            _put(p, row)
            p.step(1)
            out.append(_bits(p))
            warn = max(warn, int(p.warn_flags.max()))
        mismatch += out[0] != out[1]
        differs += out[1] != out[2]
        nonfinite += int((~np.isfinite(under_test.qvel)).sum() + (~np.isfinite(under_test.qpos)).sum())
    cap = model.opt_iterations if model.opt_iterations != si.model.opt_iterations else 0
    bound = int((iters[lo:lo + n] > cap).sum()) if cap else 0
    return mismatch, differs, bound, nonfinite, warn, owarn


def option_against_oracle(si, kind, calls, lo=LO, n=N, E=2):
    """Part B, fp64.  A default-model engine given the setter calls against the oracle built from the modified model, both
    from the default oracle's states.  Returns (worst relative dv, max contacts, steps skipped for a contact on the
    dist = 0 threshold that one side saw alone, steps whose contact counts differ otherwise, steps at which the modified
    oracle differs from the default one by more than 1e-9 of the velocity change, the largest warn flag, the oracles'
    warnings)."""
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    rows, _, owarn = _trajectory(si, lo + n + 1)
    model = _model_with(si, kind, calls)
    orc = Oracle(model, engine.make_blob(model, si.key_joint_ids))
    phys = _engine(si, 64, E)
    _apply(phys, kind, calls)
    worst, maxcon, borderline, unequal, exercised, warn = 0.0, 0, 0, 0, 0, 0
    for i in range(lo, lo + n):
        _put(phys, rows[i]); phys.step(1)
        _put_oracle(orc, rows[i]); orc.step(1)
        warn = max(warn, int(phys.warn_flags.max()))
        v0 = rows[i][1]
        scale = max(np.abs(orc.qvel - v0).max(), 1e-9)
        exercised += np.abs(orc.qvel - rows[i + 1][1]).max() / scale > 1e-9
        maxcon = max(maxcon, orc.ncon)
        ne = int(phys.get(engine.NCON)[0])
        if ne != orc.ncon:
            # (tests/test_gpu_parity.py: teacher_forced -- a contact exactly on the dist = 0 threshold may be seen by one side only)
            d_e = np.abs(phys.get(engine.CONTACT_DIST)[0][:ne].astype(np.float64))
            d_o = np.abs(orc.contact.reshape(-1, 16)[:, 0])
            if int((d_e < 1e-11).sum() + (d_o < 1e-11).sum()) < abs(ne - orc.ncon):
                unequal += 1
            else:
                borderline += 1
            continue
        qv = phys.qvel.astype(np.float64)
        assert np.array_equal(qv[0], qv[-1])   # (identical envs)
        worst = max(worst, float(np.abs(qv[0] - orc.qvel).max() / scale))
    return worst, maxcon, borderline, unequal, int(exercised), warn, owarn | orc.warnings


def mpr_settings_compared(si, precision, sequences, lo=LO, n=N, E=2):
    """Parts C1 and C2.  One engine per entry of `sequences` (each a tuple of (tolerance, polytope_tolerance) calls, in
    order; () = a default engine).  Returns (steps at which engine k differs from engine 0 in any bit, for k = 1 ..;
    then the largest warn flag and the oracle's warnings)."""
    rows, _, owarn = _trajectory(si, lo + n)
    engines = []
    for calls in sequences:
        p = _engine(si, precision, E)
        for t, pt in calls:
            p.set_mpr_tolerance(t, pt)
        engines.append(p)
    differs, warn = [0] * (len(engines) - 1), 0
    for row in rows[lo:lo + n]:
        out = []
        for p in engines:
            _put(p, row)
            p.step(1)
            out.append(_bits(p))
            warn = max(warn, int(p.warn_flags.max()))
        for k in range(1, len(engines)):
            differs[k - 1] += out[k] != out[0]
    return (*differs, warn, owarn)


def refined_rule_at(si, steps, E=2):
    """Part C3, fp64.  At each mj_step of `steps`, from the default oracle's state: the engine after (1e-6, 1e-10) against
    the oracle under set_mpr_experiment(poly_tolerance=MPR_POLY_REFINED).  Returns (worst relative dv of that pair, the
    SMALLEST relative difference between the uniform engine and the refined engine over the steps, the smallest relative
    difference between the oracle's two rules, steps with unequal contact counts, the largest warn flag, the oracles'
    warnings)."""
    from robopianist_amd import engine
    from oracle import rp_oracle
    rows, _, owarn = _trajectory(si, max(steps) + 2)
    orc = rp_oracle.Oracle(si.model, engine.make_blob(si.model, si.key_joint_ids))
    refined, uniform = _engine(si, 64, E), _engine(si, 64, E)
    refined.set_mpr_tolerance(1e-6, rp_oracle.MPR_POLY_REFINED)
    worst, branch, rules, unequal, warn = 0.0, np.inf, np.inf, 0, 0
    try:
        rp_oracle.set_mpr_experiment(poly_tolerance=rp_oracle.MPR_POLY_REFINED)
        for i in steps:
            _put_oracle(orc, rows[i]); orc.step(1)
            for p in (refined, uniform):
                _put(p, rows[i]); p.step(1)
                warn = max(warn, int(p.warn_flags.max()))
            scale = max(np.abs(orc.qvel - rows[i][1]).max(), 1e-9)
            vr, vu = refined.qvel[0].astype(np.float64), uniform.qvel[0].astype(np.float64)
            unequal += int(refined.get(engine.NCON)[0]) != orc.ncon
            worst = max(worst, float(np.abs(vr - orc.qvel).max() / scale))
            branch = min(branch, float(np.abs(vu - vr).max() / scale))
            rules = min(rules, float(np.abs(rows[i + 1][1] - orc.qvel).max() / scale))
    finally:
        rp_oracle.set_mpr_experiment()   # (process-wide: back to the uniform rule)
    return worst, branch, rules, unequal, warn, owarn | orc.warnings


# ---------------------------------------------------------------------------------------------------------------- A

_CONFIGS = [
    ("limits", ((4, 6),)), ("limits", ((3, 0),)), ("limits", ((0, 4),)), ("limits", ((4, 6), (0, 0))),
    ("tolerance", ((1e-3, 0.3),)), ("tolerance", ((1e-3, 0),)), ("tolerance", ((0, 0.3),)), ("tolerance", ((1e-3, 0.3), (0, 0))),
]


# The line-search tolerance alone rarely decides anything: with the Newton tolerance at 1e-8 the oracle's step at 0.3 leaves
# its step at 0.01 on 22 (capsule) and 25 (hull) of the replay's 1580 mj_steps, none of them in capsule rows 400..469.  These
# windows hold the densest runs of such steps (capsule: rows 324, 364, 375; hull: 879, 891, 893, 895).
_WINDOW = {("capsule", "tolerance", ((0, 0.3),)): 320, ("hull", "tolerance", ((0, 0.3),)): 830}


def _check_a(scene_name, precision, kind, calls):
    lo = _WINDOW.get((scene_name, kind, calls), LO)
    mismatch, differs, bound, nonfinite, warn, owarn = setter_equals_model_option(_scene(scene_name), precision, kind, calls, lo)
    print(f"{scene_name} fp{precision} {kind} {calls}, rows {lo}..{lo + N - 1}: {mismatch} steps differ from the model-built engine, "
          f"{differs} of {N} differ from a default engine, Newton cap bound on {bound}")
    assert warn == 0 and owarn == 0 and nonfinite == 0, (warn, owarn, nonfinite)
    assert mismatch == 0, mismatch
    assert differs >= 1, "the setting changed no step of the window"
    if kind == "limits" and calls[0][0] > 0:
        assert bound >= 10, bound


@pytest.mark.parametrize("kind,calls", _CONFIGS)
@pytest.mark.parametrize("scene_name", ["capsule", "hull"])
def test_setter_equals_the_model_option_bit_for_bit(scene_name, kind, calls):
    """rp_set_solver_limits / rp_set_solver_tolerance against the blob's opt_* values, both arguments, either alone, and
    (0, 0) afterwards leaving the setting as it was; fp64."""
    _check_a(scene_name, 64, kind, calls)


@pytest.mark.parametrize("kind,calls", [_CONFIGS[0], _CONFIGS[4]])
def test_setter_equals_the_model_option_bit_for_bit_fp32(kind, calls):
    _check_a("capsule", 32, kind, calls)


# ---------------------------------------------------------------------------------------------------------------- B

@pytest.mark.parametrize("kind,calls", [_CONFIGS[0], _CONFIGS[4]])
@pytest.mark.parametrize("scene_name", ["capsule", "hull"])
def test_capped_and_loose_solves_match_the_oracle(scene_name, kind, calls):
    """A Newton solve ending on its cap of 4 with line searches ending on 6 evaluations, and a solve at tolerance 1e-3 /
    line-search tolerance 0.3, against the oracle built from the model with the same options (wave emulator, capsule
    fingertips: 6.6e-13 and 2.2e-12)."""
    worst, maxcon, borderline, unequal, exercised, warn, owarn = option_against_oracle(_scene(scene_name), kind, calls)
    print(f"{scene_name} {kind} {calls}: worst rel dv {worst:.2e}, max contacts {maxcon}, {borderline} borderline steps, "
          f"the modified oracle leaves the default one on {exercised} of {N} steps")
    assert warn == 0 and owarn == 0, (warn, owarn)
    assert unequal == 0 and borderline <= 2, (unequal, borderline)
    assert maxcon >= 4 and exercised >= 10, (maxcon, exercised)
    assert worst < 1e-9, worst


# ---------------------------------------------------------------------------------------------------------------- C

def test_mpr_polytope_tolerance_is_reset_by_zero():
    """(0, 0) after (1e-6, 1e-3) gives the default engine's bits on every step (the Python default set_mpr_tolerance() is
    that call); (1e-6, 1e-3) itself does not.  Hull fingertips."""
    loose, reset, warn, owarn = mpr_settings_compared(_scene("hull"), 64, ((), ((1e-6, 1e-3),), ((1e-6, 1e-3), (0, 0))))
    print(f"hull: (1e-6, 1e-3) differs from default on {loose} of {N} steps; followed by (0, 0) on {reset}")
    assert warn == 0 and owarn == 0, (warn, owarn)
    assert loose >= 1, "the polytope tolerance decided no step of the window"
    assert reset == 0, reset


def test_mpr_tolerance_alone_sets_both():
    """(t > 0, p <= 0): both become t.  Cylinder knuckles and hull fingertips, so that either tolerance decides pairs:
    (1e-3, 0) equals (1e-3, 1e-3) and differs from (1e-3, 1e-6) and from the default."""
    same, poly, default, warn, owarn = mpr_settings_compared(
        _scene("cylinder"), 64, (((1e-3, 1e-3),), ((1e-3, 0),), ((1e-3, 1e-6),), ()))
    print(f"cylinder: (1e-3, 0) differs from (1e-3, 1e-3) on {same} steps; (1e-3, 1e-6) on {poly}; default on {default}")
    assert warn == 0 and owarn == 0, (warn, owarn)
    assert same == 0, same
    assert poly >= 1 and default >= 1, (poly, default)


def test_mpr_polytope_tolerance_alone_leaves_tolerance():
    """(t <= 0, p > 0): tolerance unchanged, polytope tolerance p.  (1e-3, 1e-3) then (0, 1e-6) equals (1e-3, 1e-6), which
    differs from (1e-3, 1e-3) (the polytope tolerance moved) and from the default (the tolerance stayed: this is the
    condition that `tolerance` decides a cylinder pair in the window)."""
    same, before, default, warn, owarn = mpr_settings_compared(
        _scene("cylinder"), 64, (((1e-3, 1e-6),), ((1e-3, 1e-3), (0, 1e-6)), ((1e-3, 1e-3),), ()))
    print(f"cylinder: (1e-3, 1e-3) then (0, 1e-6) differs from (1e-3, 1e-6) on {same} steps; (1e-3, 1e-3) on {before}; default on {default}")
    assert warn == 0 and owarn == 0, (warn, owarn)
    assert same == 0, same
    assert before >= 1 and default >= 1, (before, default)


def test_mpr_both_tolerances_given_set_both_and_zero_follows_tolerance():
    """(t > 0, p > 0) sets both: (1e-3, 1e-3) then (1e-6, 1e-6) is the default again.  And (0, 0) after (1e-3, 1e-6) sets
    the polytope tolerance to the CURRENT tolerance: (1e-3, 1e-3)."""
    back, loose, warn, owarn = mpr_settings_compared(_scene("cylinder"), 64, ((), ((1e-3, 1e-3), (1e-6, 1e-6)), ((1e-3, 1e-3),)))
    print(f"cylinder: (1e-3, 1e-3) then (1e-6, 1e-6) differs from default on {back} steps; (1e-3, 1e-3) on {loose}")
    assert warn == 0 and owarn == 0, (warn, owarn)
    assert back == 0, back
    assert loose >= 1, loose
    same, poly, warn, owarn = mpr_settings_compared(_scene("cylinder"), 64, (((1e-3, 1e-3),), ((1e-3, 1e-6), (0, 0)), ((1e-3, 1e-6),)))
    print(f"cylinder: (1e-3, 1e-6) then (0, 0) differs from (1e-3, 1e-3) on {same} steps; (1e-3, 1e-6) on {poly}")
    assert warn == 0 and owarn == 0, (warn, owarn)
    assert same == 0 and poly >= 1, (same, poly)


def test_mpr_tolerances_clamp_at_1e_6_in_fp32():
    """An fp32 engine after (1e-10, 1e-10) is a default fp32 engine, also when (1e-3, 1e-3) came first; (1e-3, 1e-3) is not."""
    tight, back, loose, warn, owarn = mpr_settings_compared(
        _scene("cylinder"), 32, ((), ((1e-10, 1e-10),), ((1e-3, 1e-3), (1e-10, 1e-10)), ((1e-3, 1e-3),)))
    print(f"cylinder fp32: (1e-10, 1e-10) differs from default on {tight} steps; after (1e-3, 1e-3) on {back}; (1e-3, 1e-3) on {loose}")
    assert warn == 0 and owarn == 0, (warn, owarn)
    assert tight == 0 and back == 0, (tight, back)
    assert loose >= 1, loose


@pytest.mark.parametrize("scene_name", ["hull", "mesh200"])
def test_refined_polytope_rule_matches_the_refined_oracle(scene_name):
    """Where the two rules part in the oracle, the engine after (1e-6, 1e-10) follows the refined oracle at 1e-9 and the
    uniform engine does not: the `tol_poly` branch ran."""
    worst, branch, rules, unequal, warn, owarn = refined_rule_at(_scene(scene_name), REFINED_STEPS[scene_name])
    print(f"{scene_name} steps {REFINED_STEPS[scene_name]}: refined engine against refined oracle {worst:.2e}; uniform engine "
          f"against refined engine at least {branch:.2e}; the oracle's two rules at least {rules:.2e}")
    assert warn == 0 and owarn == 0 and unequal == 0, (warn, owarn, unequal)
    assert rules > 1e-9, rules     # (the recorded steps still are steps at which the rules part)
    assert branch > 1e-9, branch
    assert worst < 1e-9, worst
