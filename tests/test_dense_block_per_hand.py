"""The lean solver stage's dense block PER HAND (csrc/rp_solver2.hpp, csrc/rp_dense.hpp; docs/LAB_NOTEBOOK.md 4g).

When no contact couples the two hands, the dirty rows of the Newton Hessian (the supports of the cross-chain contacts)
form one diagonal block per hand, and the stage factors the two blocks side by side instead of one pivot after the
other.  A contact between the hands keeps the joint block, and so does RP_DENSE_HANDS=0.  An exactly block-diagonal
matrix gives the same bits either way.

Teacher-forced against the oracle at the existing 1e-9 bar, on poses where the header of the solved system
(DEBUG_HANDOVER_HDR after rp_forward: dirty mask, capacity class) and the contact list show the shape the case is about:
  a  one hand with a finger-finger contact (replay)          b  both hands, unequal row counts (replay)
  c  a contact between the hands: joint block                d  a key pressed from two chains of a hand: a dirty slot row
  e  a palm (trunk link) in a cross contact                  f  no cross contact at all
The functions of this module are also run on the CPU wave emulator (tests/wavesim/dense_per_hand.py)."""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# replay rows (mj_steps of tests/golden/twinkle_twinkle_actions.npy, capsule fingertips) around which the shapes occur
REPLAY_WINDOW = (38, 74)      # cases a, b, f
SLOT_WINDOW = (1328, 1344)    # case d
HAND_IN_HAND_POSES = 36       # cases c, e


def make_engine(si, nenv, knob=None, blob=None):
    """An engine built with RP_DENSE_HANDS = knob (None: unset, the default)."""
    from robopianist_amd import engine
    old = os.environ.pop("RP_DENSE_HANDS", None)
    try:
        if knob is not None:
            os.environ["RP_DENSE_HANDS"] = str(knob)
        return engine.BatchedPhysics(si.model, si.key_joint_ids, n_envs=nenv, precision=64, blob=blob)
    finally:
        os.environ.pop("RP_DENSE_HANDS", None)
        if old is not None:
            os.environ["RP_DENSE_HANDS"] = old


_tables = {}


def _topology(si):
    """(tree of every link lane, is-trunk of every link lane, body -> tree or -1)."""
    if id(si) not in _tables:
        from robopianist_amd.model import engine_tables
        t = engine_tables.build_engine_tables(si.model, si.key_joint_ids)
        tree = np.asarray(t["eng_link_tree"]).astype(int)
        trunk = np.asarray(t["eng_link_depth"]).astype(int) < np.asarray(t["eng_tree_trunk"]).astype(int)[tree]
        bn = si.model.names["body"]
        hand = np.array([0 if n.startswith("rh_") else (1 if n.startswith("lh_") else -1) for n in bn])
        _tables[id(si)] = (tree, trunk, hand)
    return _tables[id(si)]


def block_shapes(phys, si):
    """Per env, from the hand-over header of the system the next solve takes (call after rp_forward) and the contact
    list: dirty link rows of either hand, dirty trunk rows, dirty slot rows, light class, contacts between the hands,
    and those of them that touch a palm."""
    from robopianist_amd import engine
    tree, trunk, hand = _topology(si)
    nl = len(tree)
    m = si.model
    bn = m.names["body"]
    hdr = phys.get(engine.DEBUG_HANDOVER_HDR)
    ncon = phys.get(engine.NCON)
    geoms = phys.get(engine.CONTACT_GEOMS)
    out = []
    for e in range(hdr.shape[0]):
        dm = (int(hdr[e, 2]) & 0xffffffff) | ((int(hdr[e, 3]) & 0xffffffff) << 32)
        rows = [L for L in range(nl) if (dm >> L) & 1]
        hh = palm = 0
        for a, b in geoms[e][:int(ncon[e])]:
            ba, bb = int(m.geom_bodyid[int(a)]), int(m.geom_bodyid[int(b)])
            if hand[ba] >= 0 and hand[bb] >= 0 and hand[ba] != hand[bb]:
                hh += 1
                palm += ("palm" in bn[ba]) or ("palm" in bn[bb])
        out.append(dict(n0=sum(1 for L in rows if tree[L] == 0), n1=sum(1 for L in rows if tree[L] == 1),
                        trunk=sum(1 for L in rows if trunk[L]), slots=bin(dm >> nl).count("1"),
                        light=int(hdr[e, 6]) == 1, hand_hand=hh, palm=palm))
    return out


_replay = {}


def replay_states(si, start, stop):
    """The oracle's own trajectory along the replay: (qpos, qvel, qacc_warmstart, ctrl) before mj_step start .. stop - 1."""
    if (id(si), start, stop) not in _replay:
        _replay[(id(si), start, stop)] = _replay_states(si, start, stop)
    return _replay[(id(si), start, stop)]


def _replay_states(si, start, stop):
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    import test_gpu_parity as tgp
    ctrl = tgp._replay_ctrl(si)
    orc = Oracle(si.model, engine.make_blob(si.model, si.key_joint_ids))
    out = []
    for s in range(stop):
        if s >= start:
            out.append((orc.qpos.copy(), orc.qvel.copy(), orc.qacc_warmstart.copy(), ctrl[s].copy()))
        orc.ctrl[:] = ctrl[s]
        orc.step(1)
    return out


def hand_in_hand_states(si, n=HAND_IN_HAND_POSES, seed=11, lo_dx=0.060, hi_dx=0.076):
    """The pile-up poses of tests/test_gpu_parity.py (forearms shifted towards each other, fingers at random postures),
    shifted less: the hands touch with a few contacts -- thumb on thumb, a thumb on the other hand's palm -- and the env
    stays in the light class."""
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    m = si.model
    jn = m.names["joint"]
    rng = np.random.default_rng(seed)
    orc = Oracle(m, engine.make_blob(m, si.key_joint_ids))
    lo, hi = m.actuator_ctrlrange[:, 0], m.actuator_ctrlrange[:, 1]
    out = []
    for _ in range(n):
        orc.reset()
        q = orc.qpos.copy()
        dx = rng.uniform(lo_dx, hi_dx)
        for i, name in enumerate(jn):
            s = name.split("/")[-1]
            if s == "forearm_tx":
                q[i] += -dx if name.startswith("rh") else dx
            elif "shadow_hand" in name and s != "forearm_ty":
                r0, r1 = m.jnt_range[i]
                q[i] = np.clip(q[i] + rng.normal(0, 0.06), r0, r1)
        v = rng.normal(0, 0.2, m.nv)
        c = lo + rng.uniform(0.2, 0.8, m.nu) * (hi - lo)
        orc.qpos[:] = q; orc.qvel[:] = v; orc.qacc_warmstart[:] = 0; orc.ctrl[:] = c
        orc.forward()   # (leaves its solution as the warm start of the step)
        out.append((q, v, orc.qacc_warmstart.copy(), c))
    return out


def _walk_replay(si, orc, start, stop):
    """Takes the oracle along the replay; yields before mj_step start .. stop - 1 (the caller steps the oracle)."""
    import test_gpu_parity as tgp
    ctrl = tgp._replay_ctrl(si)
    for s in range(stop):
        orc.ctrl[:] = ctrl[s]
        if s < start:
            orc.step(1)
        else:
            yield


def _walk_hands(si, orc):
    """Imposes the hand-in-hand poses on the oracle; yields before the step of each."""
    for q, v, _, c in hand_in_hand_states(si):
        orc.reset()
        orc.qpos[:] = q; orc.qvel[:] = v; orc.qacc_warmstart[:] = 0; orc.ctrl[:] = c
        orc.forward()   # (the step is mj_step2; mj_step1 first: the position-dependent stage of the imposed state)
        orc.qacc_warmstart[:] = 0   # (not forward's converged solution: the step's solve takes all its Newton iterations)
        yield


def teacher_forced_records(si, walk, knob=None):
    """Every state of the walk stepped once by the engine, from the oracle's state, and by the oracle.  One record per
    state: the shape of the solved system, relative velocity error, contact counts, Newton iterations and warn flags of
    both sides."""
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    phys = make_engine(si, 1, knob)
    orc = Oracle(si.model, phys.blob)
    rec = []
    for _ in walk(si, orc):
        v = orc.qvel.copy()
        phys.reset()   # (clears the sticky warn flags)
        phys.set(engine.QPOS, orc.qpos[None, :]); phys.set(engine.QVEL, orc.qvel[None, :])
        phys.set(engine.QACC_WARMSTART, orc.qacc_warmstart[None, :]); phys.set(engine.CTRL, orc.ctrl[None, :])
        phys.forward()
        r = block_shapes(phys, si)[0]
        phys.step(1); orc.step(1)
        it = int(phys.get(engine.SOLVER_ITER)[0])
        den = max(np.abs(orc.qvel - v).max(), 1e-9)
        r.update(err=float(np.abs(phys.qvel[0] - orc.qvel).max() / den), ncon=int(phys.get(engine.NCON)[0]), ncon_oracle=int(orc.ncon),
                 iters=it & 255, iters_oracle=int(orc.solver_iter), rows=(it >> 8) & 255, warn=int(phys.warn_flags.max()),
                 warn_oracle=int(orc.warnings))
        rec.append(r)
    return rec


CASES = {
    # name: (source of the states, which records show the shape, how many of them the source must hold)
    "a": ("replay", lambda r: r["light"] and r["hand_hand"] == 0 and r["slots"] == 0 and min(r["n0"], r["n1"]) == 0 and max(r["n0"], r["n1"]) >= 8, 3),
    "b": ("replay", lambda r: r["light"] and r["hand_hand"] == 0 and min(r["n0"], r["n1"]) >= 8 and r["n0"] != r["n1"], 3),
    "c": ("hands", lambda r: r["light"] and r["hand_hand"] > 0 and min(r["n0"], r["n1"]) > 0, 4),
    "d": ("slot", lambda r: r["light"] and r["hand_hand"] == 0 and r["slots"] > 0, 1),
    "e": ("hands", lambda r: r["light"] and r["palm"] > 0 and r["trunk"] > 0, 2),
    "f": ("replay", lambda r: r["light"] and r["ncon"] > 0 and r["n0"] + r["n1"] + r["slots"] == 0, 3),
}
_records = {}


def case_records(si, name, knob=None):
    """The records of the case's source (computed once per source and knob), and those that show its shape."""
    src, shape, _ = CASES[name]
    key = (id(si), src, knob)
    if key not in _records:
        walk = {"replay": lambda s_, o: _walk_replay(s_, o, *REPLAY_WINDOW), "slot": lambda s_, o: _walk_replay(s_, o, *SLOT_WINDOW),
                "hands": _walk_hands}[src]
        _records[key] = teacher_forced_records(si, walk, knob)
    return _records[key], [r for r in _records[key] if shape(r)]


def check_case(si, name, knob=None):
    rec, hits = case_records(si, name, knob)
    print(f"case {name}: {len(hits)} of {len(rec)} states show the shape; worst rel dv {max(r['err'] for r in hits) if hits else float('nan'):.2e}; "
          f"(n0, n1, slots, iterations): {[(r['n0'], r['n1'], r['slots'], r['iters']) for r in hits][:8]}")
    assert len(hits) >= CASES[name][2], (name, len(hits), [(r["n0"], r["n1"], r["slots"], r["hand_hand"], r["light"]) for r in rec])
    for r in hits:
        assert r["rows"] == r["n0"] + r["n1"] + r["slots"], r   # (the header read before the step IS the solved system)
        assert r["ncon"] == r["ncon_oracle"], r
        assert r["err"] < 1e-9, r
        assert r["iters"] == r["iters_oracle"], r
        assert r["warn"] == 0 and r["warn_oracle"] == 0, r
    return len(hits), max(r["err"] for r in hits)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_block_per_hand_matches_the_oracle(two_hand_scene, name):
    check_case(two_hand_scene, name)


def switch_states(si):
    """Start states for the switch test: of cases a, b and d, the first states that show the shape."""
    out = []
    for name, window in (("a", REPLAY_WINDOW), ("b", REPLAY_WINDOW), ("d", SLOT_WINDOW)):
        rec, _ = case_records(si, name)
        states = replay_states(si, window[0], window[1])
        idx = [i for i, r in enumerate(rec) if CASES[name][1](r)]
        assert idx, name
        out += [(name, window[0] + i, states[i]) for i in idx[:2]]
    return out


def run_switch(si, nsteps=10):
    """Ten mj_steps from every start state, along the replay's controls, under RP_DENSE_HANDS = 0 / 1 / default."""
    from robopianist_amd import engine
    import test_gpu_parity as tgp
    ctrl = tgp._replay_ctrl(si)
    starts = switch_states(si)
    E = len(starts)
    res = {}
    for knob in (0, 1, None):
        p = make_engine(si, E, knob)
        p.set(engine.QPOS, np.stack([s[2][0] for s in starts])); p.set(engine.QVEL, np.stack([s[2][1] for s in starts]))
        p.set(engine.QACC_WARMSTART, np.stack([s[2][2] for s in starts]))
        iters = []
        for t in range(nsteps):
            p.set(engine.CTRL, np.stack([ctrl[s[1] + t] for s in starts]))
            if t == 0:
                p.forward()
                shapes = block_shapes(p, si)
                for (name, _, _), r in zip(starts, shapes):
                    assert CASES[name][1](dict(r, ncon=1)), (name, r)
            p.step(1)
            iters.append(p.get(engine.SOLVER_ITER).copy())
        assert p.warn_flags.max() == 0
        res[knob] = dict(qpos=p.qpos.copy(), qvel=p.qvel.copy(), warm=p.get(engine.QACC_WARMSTART).copy(), iters=np.stack(iters))
    return res


def check_switch(si):
    res = run_switch(si)
    for f in ("qpos", "qvel", "warm", "iters"):
        assert np.array_equal(res[1][f], res[0][f]), f   # side by side: the same bits as the joint block
    assert np.array_equal(res[None]["iters"], res[0]["iters"])
    worst = 0.0
    for f in ("qpos", "qvel", "warm"):
        rel = np.abs(res[None][f] - res[0][f]).max() / np.abs(res[0][f]).max()
        worst = max(worst, rel)
        print(f"default vs RP_DENSE_HANDS=0, {f}: {rel:.2e} relative")
        assert rel < 1e-12, (f, rel)
    assert (res[0]["iters"] & 255).max() >= 2 and ((res[0]["iters"][0] >> 8) & 255).min() > 0
    return worst


def test_dense_block_switch_values_agree(two_hand_scene):
    """RP_DENSE_HANDS=1 against =0: qpos, qvel, qacc_warmstart and SOLVER_ITER bitwise equal after 10 mj_steps from
    states of cases a, b and d (an exactly block-diagonal matrix: the joint factorisation only subtracts products with
    an exact zero).  The default against =0: equal SOLVER_ITER, state within 1e-12 relative (the default is the block
    per hand: the bound leaves room for an elimination order that differs at rounding level)."""
    check_switch(two_hand_scene)


def test_dense_block_per_hand_under_every_schedule(two_hand_scene):
    """Fused substeps, and three slices with the split position stage, against one launch per stage: bit-identical, as
    the existing schedule tests require, with the dense block per hand in every light env.  (1100 envs: the engine runs
    slices from 1024 envs on.)"""
    from robopianist_amd import engine
    import test_gpu_parity as tgp
    si = two_hand_scene
    E = 1100
    ctrl = tgp._replay_ctrl(si)
    rng = np.random.default_rng(6)
    gain = 1 + 0.1 * rng.standard_normal((E, 1))
    ref = make_engine(si, E)
    ref.set_split_position_stage(False); ref.set_stream_slices(1); ref.set_fused_substeps(False)
    fused = make_engine(si, E)
    fused.set_fused_substeps(True); fused.set_stream_slices(1)
    sliced = make_engine(si, E)
    sliced.set_stream_slices(3); sliced.set_split_position_stage(True); sliced.set_fused_substeps(False)
    assert fused.fused_substeps and sliced.split_position_stage and not ref.fused_substeps
    both = 0
    for t in range(8):
        c = ctrl[10 * (t + 3)][None, :] * gain
        for p in (ref, fused, sliced):
            p.set(engine.CTRL, c)
            p.step(10)
        for p in (fused, sliced):
            assert np.array_equal(ref.qpos, p.qpos) and np.array_equal(ref.qvel, p.qvel), t
            assert np.array_equal(ref.get(engine.SOLVER_ITER), p.get(engine.SOLVER_ITER)), t
            assert np.array_equal(ref.get(engine.NCON), p.get(engine.NCON)), t
        both += sum(1 for r in block_shapes(ref, si) if r["light"] and min(r["n0"], r["n1"]) > 0 and r["hand_hand"] == 0)
    assert both > 0.05 * 8 * E, both   # (envs whose next solve takes a block per hand, of the 8 x E looked at: a presence check)
    assert max(int(p.warn_flags.max()) for p in (ref, fused, sliced)) == 0
